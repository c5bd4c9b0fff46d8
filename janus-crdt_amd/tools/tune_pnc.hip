// tune_pnc.hip — dev tool: interleaved A/B timing of PN-Counter dense-merge kernel variants on the
// C2 shape (10M keys x 64 replicas, int64), one process, hipEvents per launch, median of rounds.
// `tune_pnc <rounds> elide`: the store-elision sweep instead (granularity x share of cells changed per launch).
// Build: make -C janus-crdt_amd build/tune_pnc (hipcc -O3 --offload-arch=gfx950) ; run on the GPU box.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { std::printf("%s: %s\n", #x, hipGetErrorString(e)); std::exit(1); } } while (0)

typedef long long v2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ v2 vmax(v2 a, v2 b) {
    v2 r;
    r.x = a.x > b.x ? a.x : b.x;
    r.y = a.y > b.y ? a.y : b.y;
    return r;
}

template <bool NT> __device__ __forceinline__ v2 ld(const v2* p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}
template <bool NT> __device__ __forceinline__ void st(v2* p, v2 v) {
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// grid-stride, U vectors in flight per lane (the production kernel shape)
template <int U, bool NTL, bool NTS, int B>
__global__ __launch_bounds__(B) void k_stride(v2* AP, v2* AN, const v2* BP, const v2* BN, unsigned long long nv) {
    const unsigned long long stride = (unsigned long long)gridDim.x * B;
    unsigned long long i = (unsigned long long)blockIdx.x * B + threadIdx.x;
    for (; i + (U - 1) * stride < nv; i += U * stride) {
        v2 ap[U], an[U], bp[U], bn[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            ap[u] = ld<false>(AP + i + u * stride);
            bp[u] = ld<NTL>(BP + i + u * stride);
            an[u] = ld<false>(AN + i + u * stride);
            bn[u] = ld<NTL>(BN + i + u * stride);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            st<NTS>(AP + i + u * stride, vmax(ap[u], bp[u]));
            st<NTS>(AN + i + u * stride, vmax(an[u], bn[u]));
        }
    }
    for (; i < nv; i += stride) {
        AP[i] = vmax(AP[i], BP[i]);
        AN[i] = vmax(AN[i], BN[i]);
    }
}

// block-contiguous chunks: block b owns [b*C, (b+1)*C) vectors, C = B*U*ITER
template <int U, bool NTL, bool NTS, int B>
__global__ __launch_bounds__(B) void k_chunk(v2* AP, v2* AN, const v2* BP, const v2* BN, unsigned long long nv, unsigned long long per_block) {
    const unsigned long long beg = (unsigned long long)blockIdx.x * per_block;
    const unsigned long long end = beg + per_block < nv ? beg + per_block : nv;
    unsigned long long i = beg + threadIdx.x;
    for (; i + (U - 1) * B < end; i += U * B) {
        v2 ap[U], an[U], bp[U], bn[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            ap[u] = ld<false>(AP + i + u * B);
            bp[u] = ld<NTL>(BP + i + u * B);
            an[u] = ld<false>(AN + i + u * B);
            bn[u] = ld<NTL>(BN + i + u * B);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            st<NTS>(AP + i + u * B, vmax(ap[u], bp[u]));
            st<NTS>(AN + i + u * B, vmax(an[u], bn[u]));
        }
    }
    for (; i < end; i += B) {
        AP[i] = vmax(AP[i], BP[i]);
        AN[i] = vmax(AN[i], BN[i]);
    }
}

// reference point: plain float4-style copy of the same byte volume (read 4 arrays... write 2)
template <int B>
__global__ __launch_bounds__(B) void k_copy(v2* dst, const v2* src, unsigned long long nv) {
    const unsigned long long stride = (unsigned long long)gridDim.x * B;
    for (unsigned long long i = (unsigned long long)blockIdx.x * B + threadIdx.x; i < nv; i += stride) dst[i] = src[i];
}

// ---- store elision (`tune_pnc <rounds> elide`) ----------------------------------------------------------
// The production kernel before store elision (flat grid, one vector per lane, non-temporal, both stores
// unconditional) beside three eliding variants: a lane stores only if a lane of its aligned group of G lanes
// changed — G = 1: per lane (16 B, partial-line writes), G = 8: per 128-B line, G = 64: per wave (1 KB).
template <int B>
__global__ __launch_bounds__(B) void k_flat(v2* AP, v2* AN, const v2* BP, const v2* BN, unsigned long long nv) {
    const unsigned long long i = (unsigned long long)blockIdx.x * B + threadIdx.x;
    if (i < nv) {
        const v2 ap = ld<true>(AP + i), bp = ld<true>(BP + i), an = ld<true>(AN + i), bn = ld<true>(BN + i);
        st<true>(AP + i, vmax(ap, bp));
        st<true>(AN + i, vmax(an, bn));
    }
}

template <int G> __device__ __forceinline__ bool group_changed(unsigned long long mask, unsigned lane) {
    if constexpr (G == 64) return mask != 0;
    else return ((mask >> (lane & (64 - G))) & ((1ull << G) - 1)) != 0;
}

template <int G, int B>
__global__ __launch_bounds__(B) void k_elide(v2* AP, v2* AN, const v2* BP, const v2* BN, unsigned long long nv) {
    const unsigned long long i = (unsigned long long)blockIdx.x * B + threadIdx.x;
    const bool in = i < nv;
    v2 ap = 0, bp = 0, an = 0, bn = 0;
    if (in) ap = ld<true>(AP + i), bp = ld<true>(BP + i), an = ld<true>(AN + i), bn = ld<true>(BN + i);
    const v2 mp = vmax(ap, bp), mn = vmax(an, bn);
    const bool dp = in && (mp.x != ap.x || mp.y != ap.y), dn = in && (mn.x != an.x || mn.y != an.y);
    const unsigned lane = threadIdx.x & 63;
    bool sp = dp, sn = dn;
    if constexpr (G > 1) {
        sp = in && group_changed<G>(__ballot(dp), lane);
        sn = in && group_changed<G>(__ballot(dn), lane);
    }
    if (sp) st<true>(AP + i, mp);
    if (sn) st<true>(AN + i, mn);
}

__device__ __forceinline__ unsigned mix(unsigned long long x) {  // splitmix64 finaliser, high word
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return (unsigned)((x ^ (x >> 31)) >> 32);
}

// B for one timed launch (untimed fill): a cell holds its base + `gen` where the pattern raises it and its base
// elsewhere; A holds at most base + gen - 1 (the launch before), so exactly the pattern's cells change.  mode 0: a share `thresh` / 2^32
// of the cells, each drawn on its own (0 = none, 2^32 = all), P and N alike; mode 1: one column per key
// (R = 64: one of the key's eight 128-B lines of P and N), P only — a sender that advanced its own column.
__global__ __launch_bounds__(256) void k_fill_b(v2* BP, v2* BN, unsigned long long nv, int mode, unsigned long long thresh, long long gen) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    v2 p = 0, n = 0;
    if (mode == 1) {
        const unsigned long long key = i >> 5, c = (i & 31) * 2;  // 32 vectors = 64 cells per key
        const unsigned col = mix(key) & 63;
        p.x = col == c ? gen : 0;
        p.y = col == c + 1 ? gen : 0;
    } else {
        p.x = mix(4 * i) < thresh ? gen : 0;
        p.y = mix(4 * i + 1) < thresh ? gen : 0;
        n.x = mix(4 * i + 2) < thresh ? gen : 0;
        n.y = mix(4 * i + 3) < thresh ? gen : 0;
    }
    // on top of a random base per cell (the generation in the low 16 bits): arrays of zeros read faster than
    // counters do (a first sweep over zero-filled arrays read 20.48 GB in 2.81 ms, the bench's data in 3.26 ms)
    const v2 salt = {0x5851f42d4c957f2dll, 0x14057b7ef767814fll};
    p += v2{(long long)mix(4 * i ^ salt.x), (long long)mix(4 * i + 1 ^ salt.x)} << 16;
    n += v2{(long long)mix(4 * i ^ salt.y), (long long)mix(4 * i + 1 ^ salt.y)} << 16;
    BP[i] = p;
    BN[i] = n;
}

// Counts the vectors where a cell of B still exceeds A (a merge that skipped a store it needed).
__global__ __launch_bounds__(256) void k_count_behind(const v2* AP, const v2* AN, const v2* BP, const v2* BN, unsigned long long nv, unsigned* bad) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const v2 ap = AP[i], bp = BP[i], an = AN[i], bn = BN[i];
    if (bp.x > ap.x || bp.y > ap.y || bn.x > an.x || bn.y > an.y) atomicAdd(bad, 1u);
}

struct Variant {
    const char* name;
    void (*launch)(v2*, v2*, const v2*, const v2*, unsigned long long, hipStream_t, int);
};

int num_cus;

template <int U, bool NTL, bool NTS, int B, int PER_CU>
void L_stride(v2* a, v2* b, const v2* c, const v2* d, unsigned long long nv, hipStream_t s, int) {
    unsigned g = num_cus * PER_CU;
    hipLaunchKernelGGL((k_stride<U, NTL, NTS, B>), dim3(g), dim3(B), 0, s, a, b, c, d, nv);
}
template <int U, bool NTL, bool NTS, int B, int ITER>
void L_chunk(v2* a, v2* b, const v2* c, const v2* d, unsigned long long nv, hipStream_t s, int) {
    unsigned long long per = (unsigned long long)B * U * ITER;
    unsigned g = (unsigned)((nv + per - 1) / per);
    hipLaunchKernelGGL((k_chunk<U, NTL, NTS, B>), dim3(g), dim3(B), 0, s, a, b, c, d, nv, per);
}

void L_flat(v2* a, v2* b, const v2* c, const v2* d, unsigned long long nv, hipStream_t s, int) {
    hipLaunchKernelGGL((k_flat<256>), dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, s, a, b, c, d, nv);
}
template <int G>
void L_elide(v2* a, v2* b, const v2* c, const v2* d, unsigned long long nv, hipStream_t s, int) {
    hipLaunchKernelGGL((k_elide<G, 256>), dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, s, a, b, c, d, nv);
}

// The elision sweep: for every share of changed cells, the variants interleaved, B re-seeded (untimed) before
// every timed launch so that each launch changes that share of A; median of rounds.  The parent kernel runs
// twice in the list: the difference of its two medians is the A/A spread that a variant has to beat.
int elide_sweep(v2* AP, v2* AN, v2* BP, v2* BN, unsigned long long nv, int rounds) {
    const std::vector<Variant> vs = {
        {"parent", L_flat}, {"lane 16B", L_elide<1>}, {"line 128B", L_elide<8>}, {"wave 1KB", L_elide<64>}, {"parent (again)", L_flat},
    };
    struct Pattern { const char* name; int mode; unsigned long long thresh; };
    const Pattern ps[] = {
        {"0 %", 0, 0}, {"one column per key", 1, 0}, {"1 % of cells", 0, (1ull << 32) / 100}, {"10 % of cells", 0, (1ull << 32) / 10},
        {"50 % of cells", 0, 1ull << 31}, {"100 %", 0, 1ull << 32},
    };
    hipStream_t s;
    CK(hipStreamCreate(&s));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    if (rounds > 2000) rounds = 2000;  // the generation stays below 2^16 (k_fill_b)
    unsigned* bad;
    CK(hipMalloc(&bad, 4));
    CK(hipMemsetAsync(bad, 0, 4, s));
    long long gen = 0;
    const unsigned fill_grid = (unsigned)((nv + 255) / 256);
    hipLaunchKernelGGL(k_fill_b, dim3(fill_grid), dim3(256), 0, s, AP, AN, nv, 0, 0ull, 0ll);  // A = the cells' bases
    std::printf("C2 shape: 10M keys x 64 replicas, int64 (P and N: 4 x 5.12 GB read, up to 2 x 5.12 GB written); median of %d rounds, ms per launch\n", rounds);
    std::printf("%-20s", "changed per launch");
    for (auto& v : vs) std::printf(" %15s", v.name);
    std::printf(" %10s\n", "A/A spread");
    for (const Pattern& p : ps) {
        std::vector<std::vector<float>> t(vs.size());
        for (int r = -1; r < rounds; ++r)  // round -1 warms every variant on this pattern
            for (size_t k = 0; k < vs.size(); ++k) {
                hipLaunchKernelGGL(k_fill_b, dim3(fill_grid), dim3(256), 0, s, BP, BN, nv, p.mode, p.thresh, ++gen);
                CK(hipEventRecord(e0, s));
                vs[k].launch(AP, AN, BP, BN, nv, s, 0);
                CK(hipEventRecord(e1, s));
                CK(hipEventSynchronize(e1));
                float ms; CK(hipEventElapsedTime(&ms, e0, e1));
                if (r >= 0) t[k].push_back(ms);
                else hipLaunchKernelGGL(k_count_behind, dim3(fill_grid), dim3(256), 0, s, AP, AN, BP, BN, nv, bad);  // untimed check
            }
        std::printf("%-20s", p.name);
        std::vector<float> med;
        for (auto& v : t) {
            std::sort(v.begin(), v.end());
            med.push_back(v[v.size() / 2]);
            std::printf(" %15.3f", med.back());
        }
        std::printf(" %10.3f\n", med.back() > med[0] ? med.back() - med[0] : med[0] - med.back());
    }
    // after each variant's warm-up launch on each pattern no cell of B may exceed A
    unsigned h = 0;
    CK(hipMemcpy(&h, bad, 4, hipMemcpyDeviceToHost));
    const bool ok = h == 0;
    std::printf("vectors of A left behind B over every variant and pattern: %u%s\n", h, ok ? " (ok)" : " (WRONG)");
    return ok ? 0 : 1;
}

int main(int argc, char** argv) {
    const unsigned long long n_cells = 10000000ull * 64, nv = n_cells / 2;
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    num_cus = prop.multiProcessorCount;
    v2 *AP, *AN, *BP, *BN;
    CK(hipMalloc(&AP, nv * 16)); CK(hipMalloc(&AN, nv * 16)); CK(hipMalloc(&BP, nv * 16)); CK(hipMalloc(&BN, nv * 16));
    if (argc > 2 && std::string(argv[2]) == "elide") return elide_sweep(AP, AN, BP, BN, nv, std::atoi(argv[1]) > 0 ? std::atoi(argv[1]) : 7);
    CK(hipMemset(AP, 1, nv * 16)); CK(hipMemset(AN, 2, nv * 16)); CK(hipMemset(BP, 3, nv * 16)); CK(hipMemset(BN, 0, nv * 16));
    std::vector<Variant> vs = {
        {"stride U4 B256 g16/CU (prod r1)", L_stride<4, false, false, 256, 16>},
        {"chunk U4 B256 it4 nt both", L_chunk<4, true, true, 256, 4>},
        {"chunk U1 B256 it1 nt both", L_chunk<1, true, true, 256, 1>},
        {"chunk U1 B256 it1 plain", L_chunk<1, false, false, 256, 1>},
        {"chunk U1 B256 it1 ntload", L_chunk<1, true, false, 256, 1>},
        {"chunk U1 B256 it1 ntstore", L_chunk<1, false, true, 256, 1>},
        {"chunk U2 B256 it1 nt both", L_chunk<2, true, true, 256, 1>},
        {"chunk U1 B512 it1 nt both", L_chunk<1, true, true, 512, 1>},
        {"chunk U1 B128 it1 nt both", L_chunk<1, true, true, 128, 1>},
        {"chunk U1 B1024 it1 nt both", L_chunk<1, true, true, 1024, 1>},
        {"chunk U1 B256 it2 nt both", L_chunk<1, true, true, 256, 2>},
        {"chunk U2 B256 it2 nt both", L_chunk<2, true, true, 256, 2>},
    };
    hipStream_t s;
    CK(hipStreamCreate(&s));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 7;
    std::vector<std::vector<float>> t(vs.size());
    for (auto& v : vs) v.launch(AP, AN, BP, BN, nv, s, 0);  // warm
    CK(hipStreamSynchronize(s));
    for (int r = 0; r < rounds; ++r)
        for (size_t k = 0; k < vs.size(); ++k) {
            CK(hipEventRecord(e0, s));
            vs[k].launch(AP, AN, BP, BN, nv, s, 0);
            CK(hipEventRecord(e1, s));
            CK(hipEventSynchronize(e1));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            t[k].push_back(ms);
        }
    // copy reference: 3 x (read 16B write 16B) ~ same 48 B/cell? no: report copy GB/s separately
    std::vector<float> tc;
    for (int r = 0; r < rounds; ++r) {
        CK(hipEventRecord(e0, s));
        hipLaunchKernelGGL((k_copy<256>), dim3(num_cus * 16), dim3(256), 0, s, AP, BP, nv);
        hipLaunchKernelGGL((k_copy<256>), dim3(num_cus * 16), dim3(256), 0, s, AN, BN, nv);
        CK(hipEventRecord(e1, s));
        CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        tc.push_back(ms);
    }
    const double bytes = (double)n_cells * 48;
    for (size_t k = 0; k < vs.size(); ++k) {
        auto v = t[k]; std::sort(v.begin(), v.end());
        std::printf("%-40s median %.3f ms  min %.3f  -> %.0f GB/s (%.1f%% of 8 TB/s)\n", vs[k].name, v[v.size() / 2], v[0],
                    bytes / (v[v.size() / 2] * 1e-3) / 1e9, 100.0 * bytes / (v[v.size() / 2] * 1e-3) / 8e12);
    }
    std::sort(tc.begin(), tc.end());
    const double cb = (double)nv * 16 * 4;
    std::printf("%-40s median %.3f ms -> %.0f GB/s (copy of 2 x 5.12 GB)\n", "reference copy", tc[tc.size() / 2], cb / (tc[tc.size() / 2] * 1e-3) / 1e9);
    return 0;
}
