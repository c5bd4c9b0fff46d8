// tune_pnc.hip — dev tool: interleaved A/B timing of PN-Counter dense-merge kernel variants on the
// C2 shape (10M keys x 64 replicas, int64), one process, hipEvents per launch, median of rounds.
// `tune_pnc <rounds> elide`: the store-elision sweep instead (granularity x share of cells changed per launch).
// `tune_pnc <rounds> steady`: the read-only steady state bench.py times (data x cadence, then the read-side shapes).
// `tune_pnc <rounds> filter`: the merge by the 32-bit shadow (csrc/pnc_dense_kernels.hpp, the library's own kernels
// in several shapes) and its build launch beside the parent's kernel.
// `tune_pnc <rounds> narrow`: the same merge of a batch held as 4-byte codes (the narrow form) in 2- and 4-cell shapes
// beside the wide batch's kernel.
// Build: make -C janus-crdt_amd build/tune_pnc (hipcc -O3 --offload-arch=gfx950) ; run on the GPU box.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "layout.hpp"
#include "pnc_dense_kernels.hpp"

using namespace jg::filt;  // the library's kernels, their shape constants and group_any

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
        sp = in && group_any<G>(__ballot(dp), lane);
        sn = in && group_any<G>(__ballot(dn), lane);
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

// ---- read-only steady state (`tune_pnc <rounds> steady`) -------------------------------------------------
// The regime bench.py times: launches back to back on a batch that is already merged, so a launch reads the four
// arrays and stores nothing.  Part 1 sets the elide sweep's protocol (one launch per event pair behind a fill of
// B, the tool's cells) beside bench.py's (5 untimed launches, then 20 between one event pair, k_synth_pnc's cells).
// Part 2 times read-side shapes of the per-line-eliding kernel in the bench's regime and, behind a fill as in the
// elide sweep, on the one-column and the 100 % pattern.

constexpr unsigned long long kBenchSeed = 0x4A414E5553ull;  // bench.py SEED

__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31; return x;
}

// csrc/synth.hip k_synth_pnc's cell i of array `which` (0 local P, 1 local N, 2 received P, 3 received N)
__device__ __forceinline__ long long synth_cell(unsigned long long i, unsigned which) {
    const unsigned long long h = mix64(kBenchSeed + (((i << 2) | which) + 1) * 0x9E3779B97F4A7C15ull);
    if (h % 100 < 30) return which < 2 ? 0 : (long long)(1ull << 63);
    return (long long)((h >> 33) % 2147483647ull);
}

__global__ __launch_bounds__(256) void k_synth(v2* X, v2* Y, unsigned long long nv, unsigned which0) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    X[i] = v2{synth_cell(2 * i, which0), synth_cell(2 * i + 1, which0)};
    Y[i] = v2{synth_cell(2 * i, which0 + 1), synth_cell(2 * i + 1, which0 + 1)};
}

__device__ __forceinline__ bool vdiff(v2 a, v2 b) { return a.x != b.x || a.y != b.y; }

// One trip of a workgroup over both counters: U vectors of each array per lane at base + u * B + thread, so a
// wave-instruction reads 1 KB contiguous and an aligned group of 8 lanes is one 128-B line; every load is issued
// before the first use.  `base` is the same in every lane of the workgroup (the ballots need whole waves).
template <int U, int B, bool NTA, bool NTB>
__device__ __forceinline__ void trip_pn(v2* AP, v2* AN, const v2* BP, const v2* BN, unsigned long long base, unsigned long long nv) {
    v2 ap[U], bp[U], an[U], bn[U];
    bool in[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const unsigned long long i = base + u * B + threadIdx.x;
        in[u] = i < nv;
        ap[u] = bp[u] = an[u] = bn[u] = 0;
        if (in[u]) ap[u] = ld<NTA>(AP + i), bp[u] = ld<NTB>(BP + i), an[u] = ld<NTA>(AN + i), bn[u] = ld<NTB>(BN + i);
    }
    const unsigned lane = threadIdx.x & 63;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const unsigned long long i = base + u * B + threadIdx.x;
        const v2 mp = vmax(ap[u], bp[u]), mn = vmax(an[u], bn[u]);
        const unsigned long long cp = __ballot(in[u] && vdiff(mp, ap[u])), cn = __ballot(in[u] && vdiff(mn, an[u]));
        if (in[u] && group_any<8>(cp, lane)) st<true>(AP + i, mp);
        if (in[u] && group_any<8>(cn, lane)) st<true>(AN + i, mn);
    }
}

// The same trip over one counter (the two-streams variants).
template <int U, int B>
__device__ __forceinline__ void trip_one(v2* A, const v2* Bv, unsigned long long base, unsigned long long nv) {
    v2 a[U], b[U];
    bool in[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const unsigned long long i = base + u * B + threadIdx.x;
        in[u] = i < nv;
        a[u] = b[u] = 0;
        if (in[u]) a[u] = ld<true>(A + i), b[u] = ld<true>(Bv + i);
    }
    const unsigned lane = threadIdx.x & 63;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const unsigned long long i = base + u * B + threadIdx.x;
        const v2 m = vmax(a[u], b[u]);
        const unsigned long long c = __ballot(in[u] && vdiff(m, a[u]));
        if (in[u] && group_any<8>(c, lane)) st<true>(A + i, m);
    }
}

// flat grid: workgroup b takes the B * U vectors from b * B * U
template <int U, int B, bool NTA, bool NTB>
__global__ __launch_bounds__(B) void k_rflat(v2* AP, v2* AN, const v2* BP, const v2* BN, unsigned long long nv) {
    trip_pn<U, B, NTA, NTB>(AP, AN, BP, BN, (unsigned long long)blockIdx.x * (B * U), nv);
}

// bounded grid, grid-stride walk: trips of B * U vectors, gridDim.x trips apart (k_stride with elision)
template <int U, int B>
__global__ __launch_bounds__(B) void k_rstride(v2* AP, v2* AN, const v2* BP, const v2* BN, unsigned long long nv) {
    const unsigned long long step = (unsigned long long)gridDim.x * (B * U);
    for (unsigned long long base = (unsigned long long)blockIdx.x * (B * U); base < nv; base += step) trip_pn<U, B, true, true>(AP, AN, BP, BN, base, nv);
}

// bounded grid, block-chunk walk: workgroup b owns [b * per_block, (b + 1) * per_block) (k_chunk with elision);
// per_block is a multiple of B * U, so trips stay line-aligned
template <int U, int B>
__global__ __launch_bounds__(B) void k_rchunk(v2* AP, v2* AN, const v2* BP, const v2* BN, unsigned long long nv, unsigned long long per_block) {
    const unsigned long long beg = (unsigned long long)blockIdx.x * per_block;
    const unsigned long long end = beg + per_block < nv ? beg + per_block : nv;
    for (unsigned long long base = beg; base < end; base += B * U) trip_pn<U, B, true, true>(AP, AN, BP, BN, base, end);
}

// two streams at a time, by halves of the grid: workgroups [0, half) merge P, [half, 2 * half) merge N
template <int U, int B>
__global__ __launch_bounds__(B) void k_rhalves(v2* AP, v2* AN, const v2* BP, const v2* BN, unsigned long long nv, unsigned half) {
    const bool isN = blockIdx.x >= half;
    trip_one<U, B>(isN ? AN : AP, isN ? BN : BP, (unsigned long long)(blockIdx.x - (isN ? half : 0)) * (B * U), nv);
}

// two streams at a time, per workgroup: P of the workgroup's B * U vectors, then N of the same vectors
template <int U, int B>
__global__ __launch_bounds__(B) void k_rpn(v2* AP, v2* AN, const v2* BP, const v2* BN, unsigned long long nv) {
    const unsigned long long base = (unsigned long long)blockIdx.x * (B * U);
    trip_one<U, B>(AP, BP, base, nv);
    trip_one<U, B>(AN, BN, base, nv);
}

// LDS-DMA: the four vectors go global -> LDS (each wave fills its own 1 KB of each array's image, base + lane x 16 B)
// and are read back by the lane that asked for them; the barrier drains the loads.  AUX: the loads' cache policy
// bits (0 default, 2 non-temporal).
typedef __attribute__((address_space(1))) const void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
template <int B, unsigned AUX>
__global__ __launch_bounds__(B) void k_rlds(v2* AP, v2* AN, const v2* BP, const v2* BN, unsigned long long nv) {
    __shared__ v2 img[4][B];
    const unsigned long long i = (unsigned long long)blockIdx.x * B + threadIdx.x;
    const bool in = i < nv;
    const unsigned w0 = threadIdx.x & ~63u, lane = threadIdx.x & 63;
    if (in) {
        __builtin_amdgcn_global_load_lds((gptr_t)(AP + i), (lptr_t)&img[0][w0], 16, 0, AUX);
        __builtin_amdgcn_global_load_lds((gptr_t)(BP + i), (lptr_t)&img[1][w0], 16, 0, AUX);
        __builtin_amdgcn_global_load_lds((gptr_t)(AN + i), (lptr_t)&img[2][w0], 16, 0, AUX);
        __builtin_amdgcn_global_load_lds((gptr_t)(BN + i), (lptr_t)&img[3][w0], 16, 0, AUX);
    }
    __syncthreads();
    v2 ap = 0, bp = 0, an = 0, bn = 0;
    if (in) ap = img[0][threadIdx.x], bp = img[1][threadIdx.x], an = img[2][threadIdx.x], bn = img[3][threadIdx.x];
    const v2 mp = vmax(ap, bp), mn = vmax(an, bn);
    const unsigned long long cp = __ballot(in && vdiff(mp, ap)), cn = __ballot(in && vdiff(mn, an));
    if (in && group_any<8>(cp, lane)) st<true>(AP + i, mp);
    if (in && group_any<8>(cn, lane)) st<true>(AN + i, mn);
}

// The library's own k_merge_dense<8> (csrc/pnc_dense_kernels.hpp) on the library's grid (halves_of).  Until round 12 this
// row timed a hand copy of the kernel's round-7 body, four streams per workgroup: profiles/r08's figures are that shape's.
void L_lib(v2* a, v2* b, const v2* c, const v2* d, unsigned long long nv, hipStream_t s, int) {
    const jg::Halves h = jg::halves_of(nv * 2, 2, (uint64_t)kDenseVecs * kDenseBlock);
    hipLaunchKernelGGL(k_merge_dense<8>, dim3(2 * (unsigned)h.blocks), dim3(kDenseBlock), 0, s, (uint4*)a, (uint4*)b, (const uint4*)c,
                       (const uint4*)d, h.n_units, h.tail, (unsigned)h.blocks);
}

unsigned blocks_of(unsigned long long nv, unsigned long long per) { return (unsigned)((nv + per - 1) / per); }

template <int U, int B, bool NTA, bool NTB>
void L_rflat(v2* a, v2* b, const v2* c, const v2* d, unsigned long long nv, hipStream_t s, int) {
    hipLaunchKernelGGL((k_rflat<U, B, NTA, NTB>), dim3(blocks_of(nv, B * U)), dim3(B), 0, s, a, b, c, d, nv);
}
template <int U, int B, int PER_CU>
void L_rstride(v2* a, v2* b, const v2* c, const v2* d, unsigned long long nv, hipStream_t s, int) {
    hipLaunchKernelGGL((k_rstride<U, B>), dim3(std::min(blocks_of(nv, B * U), (unsigned)(num_cus * PER_CU))), dim3(B), 0, s, a, b, c, d, nv);
}
template <int U, int B, int PER_CU>
void L_rchunk(v2* a, v2* b, const v2* c, const v2* d, unsigned long long nv, hipStream_t s, int) {
    const unsigned long long trip = B * U, want = (unsigned long long)num_cus * PER_CU;
    const unsigned long long per = std::max<unsigned long long>((nv + want * trip - 1) / (want * trip), 1) * trip;
    hipLaunchKernelGGL((k_rchunk<U, B>), dim3(blocks_of(nv, per)), dim3(B), 0, s, a, b, c, d, nv, per);
}
template <int U, int B>
void L_rhalves(v2* a, v2* b, const v2* c, const v2* d, unsigned long long nv, hipStream_t s, int) {
    const unsigned half = (unsigned)jg::halves_of(nv, 1, B * U).blocks;
    hipLaunchKernelGGL((k_rhalves<U, B>), dim3(2 * half), dim3(B), 0, s, a, b, c, d, nv, half);
}
template <int U, int B>
void L_rpn(v2* a, v2* b, const v2* c, const v2* d, unsigned long long nv, hipStream_t s, int) {
    hipLaunchKernelGGL((k_rpn<U, B>), dim3(blocks_of(nv, B * U)), dim3(B), 0, s, a, b, c, d, nv);
}
template <int B, unsigned AUX>
void L_rlds(v2* a, v2* b, const v2* c, const v2* d, unsigned long long nv, hipStream_t s, int) {
    hipLaunchKernelGGL((k_rlds<B, AUX>), dim3(blocks_of(nv, B)), dim3(B), 0, s, a, b, c, d, nv);
}

float median(std::vector<float> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

int steady_sweep(v2* AP, v2* AN, v2* BP, v2* BN, unsigned long long nv, int rounds) {
    hipStream_t s;
    CK(hipStreamCreate(&s));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    if (rounds > 500) rounds = 500;  // the generation stays below 2^16 (k_fill_b)
    unsigned* bad;
    CK(hipMalloc(&bad, 4));
    CK(hipMemsetAsync(bad, 0, 4, s));
    long long gen = 0;
    const unsigned g256 = (unsigned)((nv + 255) / 256);
    const Variant parent = {"flat U1 B256 (parent)", L_elide<8>};

    // data: the tool's cells (A = B = the bases, so a fill at 0 % rewrites B's values) or the bench's (A merged once)
    const auto set_data = [&](bool bench) {
        if (bench) {
            hipLaunchKernelGGL(k_synth, dim3(g256), dim3(256), 0, s, AP, AN, nv, 0u);
            hipLaunchKernelGGL(k_synth, dim3(g256), dim3(256), 0, s, BP, BN, nv, 2u);
            parent.launch(AP, AN, BP, BN, nv, s, 0);
        } else {
            hipLaunchKernelGGL(k_fill_b, dim3(g256), dim3(256), 0, s, AP, AN, nv, 0, 0ull, 0ll);
            hipLaunchKernelGGL(k_fill_b, dim3(g256), dim3(256), 0, s, BP, BN, nv, 0, 0ull, 0ll);
        }
    };
    // interleaved: an untimed write-only fill of B, then one launch between an event pair (the elide sweep)
    const auto t_interleaved = [&](const Variant& v, bool bench, int mode, unsigned long long thresh) {
        if (bench) hipLaunchKernelGGL(k_synth, dim3(g256), dim3(256), 0, s, BP, BN, nv, 2u);
        else hipLaunchKernelGGL(k_fill_b, dim3(g256), dim3(256), 0, s, BP, BN, nv, mode, thresh, ++gen);
        CK(hipEventRecord(e0, s));
        v.launch(AP, AN, BP, BN, nv, s, 0);
        CK(hipEventRecord(e1, s));
        CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        return ms;
    };
    // back to back: 5 untimed launches, a fence, 20 launches between one event pair (bench.py timed())
    const auto t_b2b = [&](const Variant& v) {
        for (int i = 0; i < 5; ++i) v.launch(AP, AN, BP, BN, nv, s, 0);
        CK(hipStreamSynchronize(s));
        CK(hipEventRecord(e0, s));
        for (int i = 0; i < 20; ++i) v.launch(AP, AN, BP, BN, nv, s, 0);
        CK(hipEventRecord(e1, s));
        CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        return ms / 20;
    };
    const auto check = [&] { hipLaunchKernelGGL(k_count_behind, dim3(g256), dim3(256), 0, s, AP, AN, BP, BN, nv, bad); };

    std::printf("C2 shape: 10M keys x 64 replicas, int64; every launch reads 4 x 5.12 GB; median of %d rounds, ms per launch\n\n", rounds);
    std::printf("Part 1: the parent kernel (k_elide<8,256>), nothing changed; A/A = the same kernel timed twice per round\n");
    std::printf("%-28s %12s %8s %14s %8s\n", "data", "interleaved", "A/A", "back to back", "A/A");
    for (int bench = 0; bench < 2; ++bench) {
        set_data(bench);
        std::vector<float> ti[2], tb[2];
        for (int r = -1; r < rounds; ++r)
            for (int k = 0; k < 2; ++k) {
                const float a = t_interleaved(parent, bench, 0, 0), b = t_b2b(parent);
                if (r >= 0) ti[k].push_back(a), tb[k].push_back(b);
            }
        const float i0 = median(ti[0]), i1 = median(ti[1]), b0 = median(tb[0]), b1 = median(tb[1]);
        std::printf("%-28s %12.3f %8.3f %14.3f %8.3f\n", bench ? "bench (k_synth_pnc, merged)" : "tool (k_fill_b bases)", i0, std::fabs(i1 - i0), b0, std::fabs(b1 - b0));
    }

    const std::vector<Variant> vs = {
        parent,
        {"csrc/pnc.hip's own body", L_lib},  // the label of the earlier tables, kept: now pnc_dense_kernels.hpp's k_merge_dense<8>
        {"flat U2 B256",L_rflat<2, 256, true, true>},
        {"flat U4 B256", L_rflat<4, 256, true, true>},
        {"flat U1 B512", L_rflat<1, 512, true, true>},
        {"flat U1 B1024", L_rflat<1, 1024, true, true>},
        {"flat U2 B512", L_rflat<2, 512, true, true>},
        {"flat U4 B1024", L_rflat<4, 1024, true, true>},
        {"stride U4 B256 8/CU (16KB)", L_rstride<4, 256, 8>},
        {"stride U2 B256 8/CU (8KB)", L_rstride<2, 256, 8>},
        {"stride U4 B1024 2/CU (64KB)", L_rstride<4, 1024, 2>},
        {"stride U1 B256 8/CU (4KB)", L_rstride<1, 256, 8>},
        {"chunk U4 B256 8/CU", L_rchunk<4, 256, 8>},
        {"chunk U2 B256 8/CU", L_rchunk<2, 256, 8>},
        {"chunk U4 B256 64/CU", L_rchunk<4, 256, 64>},
        {"halves P|N U1 B256", L_rhalves<1, 256>},
        {"halves P|N U2 B256", L_rhalves<2, 256>},
        {"P then N U2 B256", L_rpn<2, 256>},
        {"P then N U4 B256", L_rpn<4, 256>},
        {"flat U1 B256 A plain B nt", L_rflat<1, 256, false, true>},
        {"flat U1 B256 A nt B plain", L_rflat<1, 256, true, false>},
        {"flat U1 B256 both plain", L_rflat<1, 256, false, false>},
        {"lds-dma U1 B256 default", L_rlds<256, 0>},
        {"lds-dma U1 B256 nt", L_rlds<256, 2>},
        {"flat U1 B256 (parent again)", L_elide<8>},
    };
    const size_t nvar = vs.size();
    std::vector<std::vector<float>> t0(nvar), t1(nvar), t2(nvar);
    // 0 % changed: the bench's data, back to back
    set_data(true);
    for (int r = -1; r < rounds; ++r)
        for (size_t k = 0; k < nvar; ++k) {
            const float ms = t_b2b(vs[k]);
            if (r >= 0) t0[k].push_back(ms);
            else check();
        }
    // one column per key and 100 %: the tool's data, each launch behind the fill that raises the pattern's cells
    set_data(false);
    for (int pat = 0; pat < 2; ++pat)
        for (int r = -1; r < rounds; ++r)
            for (size_t k = 0; k < nvar; ++k) {
                const float ms = pat == 0 ? t_interleaved(vs[k], false, 1, 0) : t_interleaved(vs[k], false, 0, 1ull << 32);
                if (r >= 0) (pat == 0 ? t1 : t2)[k].push_back(ms);
                else check();
            }
    std::printf("\nPart 2: read-side shapes, per-line store elision in all of them\n");
    std::printf("%-30s %22s %22s %22s\n", "", "0 % (bench data,", "one column per key", "100 %");
    std::printf("%-30s %22s %22s %22s\n", "variant", "back to back)", "(behind a fill)", "(behind a fill)");
    for (size_t k = 0; k < nvar; ++k) std::printf("%-30s %22.3f %22.3f %22.3f\n", vs[k].name, median(t0[k]), median(t1[k]), median(t2[k]));
    std::printf("%-30s %22.3f %22.3f %22.3f\n", "A/A spread (parent twice)", std::fabs(median(t0[0]) - median(t0[nvar - 1])),
                std::fabs(median(t1[0]) - median(t1[nvar - 1])), std::fabs(median(t2[0]) - median(t2[nvar - 1])));
    std::printf("%-30s %22.3f %22.3f %22.3f\n", "parent, min of rounds", *std::min_element(t0[0].begin(), t0[0].end()),
                *std::min_element(t1[0].begin(), t1[0].end()), *std::min_element(t2[0].begin(), t2[0].end()));
    std::printf("%-30s %22.3f %22.3f %22.3f\n", "parent, max of rounds", *std::max_element(t0[0].begin(), t0[0].end()),
                *std::max_element(t1[0].begin(), t1[0].end()), *std::max_element(t2[0].begin(), t2[0].end()));
    unsigned h = 0;
    CK(hipMemcpy(&h, bad, 4, hipMemcpyDeviceToHost));
    const bool ok = h == 0;
    std::printf("vectors of A left behind B over every variant and pattern: %u%s\n", h, ok ? " (ok)" : " (WRONG)");
    return ok ? 0 : 1;
}

// ---- the merge by the 32-bit shadow (`tune_pnc <rounds> filter`) ------------------------------------------------
// The bench's data (k_synth_pnc's cells, A merged once) throughout.  0 %: launches back to back on the merged batch
// (bench.py's protocol).  One column per key and 100 %: each timed launch behind an untimed fill of B that raises the
// pattern's cells above everything A holds and, for a kernel that reads the shadow, an untimed clamp pass that makes
// the shadow exact for what the launches before it left in A (the variants share A).  The parent (the halves grid of
// k_merge_dense) runs first and last: the difference of its two medians is the A/A spread.

// B for one timed launch: the synthetic received cell, or where the pattern raises it a value above every earlier one
// that still fits 32 bits (0x7FFE0000 + gen, gen < 2^16; the 6e-5 of the cells whose own value is larger stay).
// mode 1: one column per key, P only; mode 2: every cell of P and N.
__global__ __launch_bounds__(256) void k_fill_f(v2* BP, v2* BN, unsigned long long nv, int mode, long long gen) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    v2 p = {synth_cell(2 * i, 2), synth_cell(2 * i + 1, 2)}, n = {synth_cell(2 * i, 3), synth_cell(2 * i + 1, 3)};
    const long long up = 0x7FFE0000ll + gen;
    if (mode == 1) {
        const unsigned long long key = i >> 5, c = (i & 31) * 2;  // 32 vectors = 64 cells per key
        const unsigned col = mix(key) & 63;
        if (col == c) p.x = up;
        if (col == c + 1) p.y = up;
    } else if (mode == 2) {
        p = v2{up, up}, n = v2{up, up};
    }
    BP[i] = p;
    BN[i] = n;
}

// Counts the cells whose shadow is not the clamp of the cell (a filtered launch that left the shadow behind A).
__global__ __launch_bounds__(256) void k_count_shadow(const long long* A, const int* S, unsigned long long n, unsigned* bad) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n && S[i] != jg::filt::clamp32(A[i])) atomicAdd(bad, 1u);
}

struct FVariant {
    const char* name;
    bool shadow;  // reads (and keeps) SP / SN
    void (*launch)(v2*, v2*, int*, int*, const v2*, const v2*, unsigned long long, hipStream_t);
};

void LF_parent(v2* ap, v2* an, int*, int*, const v2* bp, const v2* bn, unsigned long long n_cells, hipStream_t s) {
    L_rhalves<1, 256>(ap, an, bp, bn, n_cells / 2, s, 0);
}
template <int CPL, int VECS, int BLOCK>
void LF(v2* ap, v2* an, int* sp, int* sn, const v2* bp, const v2* bn, unsigned long long n_cells, hipStream_t s) {
    const jg::Halves h = jg::halves_of(n_cells, CPL, (uint64_t)VECS * BLOCK);
    hipLaunchKernelGGL((jg::filt::k_merge_filtered<CPL, VECS, BLOCK>), dim3(2 * (unsigned)h.blocks), dim3(BLOCK), 0, s, (long long*)ap,
                       (long long*)an, sp, sn, (const long long*)bp, (const long long*)bn, h.n_units, h.tail, (unsigned)h.blocks);
}
void LF_build(v2* ap, v2* an, int* sp, int* sn, const v2* bp, const v2* bn, unsigned long long n_cells, hipStream_t s) {
    const jg::Halves h = jg::halves_of(n_cells, 2, kBuildBlock);
    hipLaunchKernelGGL(jg::filt::k_merge_build<kBuildBlock>, dim3(2 * (unsigned)h.blocks), dim3(kBuildBlock), 0, s, (long long*)ap, (long long*)an,
                       sp, sn, (const long long*)bp, (const long long*)bn, h.n_units, h.tail, (unsigned)h.blocks);
}

int filter_sweep(v2* AP, v2* AN, v2* BP, v2* BN, unsigned long long nv, int rounds) {
    const unsigned long long n_cells = nv * 2;
    hipStream_t s;
    CK(hipStreamCreate(&s));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    if (rounds > 500) rounds = 500;  // the generation stays below 2^16 (k_fill_f)
    int *SP, *SN;
    CK(hipMalloc(&SP, n_cells * 4)); CK(hipMalloc(&SN, n_cells * 4));
    unsigned* bad;  // [0] cells of A behind B, [1] cells whose shadow is not their clamp
    CK(hipMalloc(&bad, 8));
    CK(hipMemsetAsync(bad, 0, 8, s));
    const unsigned g256 = (unsigned)((nv + 255) / 256), gc = (unsigned)((n_cells + 255) / 256);
    const std::vector<FVariant> vs = {
        {"parent (halves U1 B256)", false, LF_parent},
        {"filtered 2 cells U1 B256", true, LF<2, 1, 256>},
        {"filtered 2 cells U2 B256", true, LF<2, 2, 256>},
        {"filtered 2 cells U4 B256", true, LF<2, 4, 256>},
        {"filtered 2 cells U1 B512", true, LF<kFiltCells, kFiltVecs, kFiltBlock>},  // the library's shape
        {"filtered 4 cells U1 B256", true, LF<4, 1, 256>},
        {"filtered 4 cells U2 B256", true, LF<4, 2, 256>},
        {"filtered 4 cells U1 B512", true, LF<4, 1, 512>},
        {"build launch (2 cells B256)", true, LF_build},  // the library's (kBuildBlock)
        {"parent (again)", false, LF_parent},
    };
    const size_t nvar = vs.size();
    const auto clamp_all = [&] {
        hipLaunchKernelGGL(jg::filt::k_shadow_clamp, dim3(num_cus * 16), dim3(256), 0, s, (const long long*)AP, SP, 0ull, n_cells);
        hipLaunchKernelGGL(jg::filt::k_shadow_clamp, dim3(num_cus * 16), dim3(256), 0, s, (const long long*)AN, SN, 0ull, n_cells);
    };
    const auto check = [&](const FVariant& v) {
        hipLaunchKernelGGL(k_count_behind, dim3(g256), dim3(256), 0, s, AP, AN, BP, BN, nv, bad);
        if (v.shadow) {
            hipLaunchKernelGGL(k_count_shadow, dim3(gc), dim3(256), 0, s, (const long long*)AP, SP, n_cells, bad + 1);
            hipLaunchKernelGGL(k_count_shadow, dim3(gc), dim3(256), 0, s, (const long long*)AN, SN, n_cells, bad + 1);
        }
    };
    const auto launch = [&](const FVariant& v) { v.launch(AP, AN, SP, SN, BP, BN, n_cells, s); };
    // the bench's data: A merged once, its shadow exact
    hipLaunchKernelGGL(k_synth, dim3(g256), dim3(256), 0, s, AP, AN, nv, 0u);
    hipLaunchKernelGGL(k_synth, dim3(g256), dim3(256), 0, s, BP, BN, nv, 2u);
    launch(vs[0]);
    clamp_all();
    std::vector<std::vector<float>> t0(nvar), t1(nvar), t2(nvar);
    for (int r = -1; r < rounds; ++r)  // 0 %: 5 untimed launches, a fence, 20 launches between one event pair
        for (size_t k = 0; k < nvar; ++k) {
            for (int i = 0; i < 5; ++i) launch(vs[k]);
            CK(hipStreamSynchronize(s));
            CK(hipEventRecord(e0, s));
            for (int i = 0; i < 20; ++i) launch(vs[k]);
            CK(hipEventRecord(e1, s));
            CK(hipEventSynchronize(e1));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            if (r >= 0) t0[k].push_back(ms / 20);
            else check(vs[k]);
        }
    long long gen = 0;
    for (int pat = 1; pat <= 2; ++pat)
        for (int r = -1; r < rounds; ++r)
            for (size_t k = 0; k < nvar; ++k) {
                hipLaunchKernelGGL(k_fill_f, dim3(g256), dim3(256), 0, s, BP, BN, nv, pat, ++gen);
                if (vs[k].shadow) clamp_all();
                CK(hipEventRecord(e0, s));
                launch(vs[k]);
                CK(hipEventRecord(e1, s));
                CK(hipEventSynchronize(e1));
                float ms; CK(hipEventElapsedTime(&ms, e0, e1));
                if (r >= 0) (pat == 1 ? t1 : t2)[k].push_back(ms);
                else check(vs[k]);
            }
    std::printf("C2 shape: 10M keys x 64 replicas, int64, the bench's cells (A merged once); median of %d rounds, ms per launch\n", rounds);
    std::printf("%-30s %22s %22s %22s\n", "", "0 % (back to back)", "one column per key", "100 %");
    std::printf("%-30s %22s %22s %22s\n", "variant", "", "(behind a fill)", "(behind a fill)");
    for (size_t k = 0; k < nvar; ++k) std::printf("%-30s %22.3f %22.3f %22.3f\n", vs[k].name, median(t0[k]), median(t1[k]), median(t2[k]));
    const float aa[3] = {std::fabs(median(t0[0]) - median(t0[nvar - 1])), std::fabs(median(t1[0]) - median(t1[nvar - 1])),
                         std::fabs(median(t2[0]) - median(t2[nvar - 1]))};
    std::printf("%-30s %22.3f %22.3f %22.3f\n", "A/A spread (parent twice)", aa[0], aa[1], aa[2]);
    std::printf("%-30s %22.3f %22.3f %22.3f\n", "parent, min of rounds", *std::min_element(t0[0].begin(), t0[0].end()),
                *std::min_element(t1[0].begin(), t1[0].end()), *std::min_element(t2[0].begin(), t2[0].end()));
    std::printf("%-30s %22.3f %22.3f %22.3f\n", "parent, max of rounds", *std::max_element(t0[0].begin(), t0[0].end()),
                *std::max_element(t1[0].begin(), t1[0].end()), *std::max_element(t2[0].begin(), t2[0].end()));
    unsigned h[2] = {0, 0};
    CK(hipMemcpy(h, bad, 8, hipMemcpyDeviceToHost));
    const bool ok = h[0] == 0 && h[1] == 0;
    std::printf("vectors of A left behind B over every variant and pattern: %u; cells whose shadow is not their clamp: %u%s\n", h[0], h[1],
                ok ? " (ok)" : " (WRONG)");
    return ok ? 0 : 1;
}

// ---- the merge of a narrow batch (`tune_pnc <rounds> narrow`) -------------------------------------------------------
// The `filter` mode's data and three patterns with B held twice: wide (BP / BN) and as the narrow form's 4-byte codes
// (CP / CN, rewritten untimed behind every fill).  The parent's wide-batch kernel (the library's filtered shape
// reading 8-byte cells of B) runs first and last: the difference of its two medians is the A/A spread.  The variants
// between read the codes in 2- and 4-cell shapes at 256 and 512 lanes; the build launch and the unfiltered kernel's
// narrow instantiation are not shaped here (they run once per cold spell).
__global__ __launch_bounds__(256) void k_codes(const long long* B, int* C, unsigned long long n, unsigned* bad) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (!jg::filt::fits(B[i])) atomicAdd(bad, 1u);
    C[i] = jg::filt::narrow(B[i]);
}

struct NVariant {
    const char* name;
    void (*launch)(v2*, v2*, int*, int*, const v2*, const v2*, const int*, const int*, unsigned long long, hipStream_t);
};
void LN_parent(v2* ap, v2* an, int* sp, int* sn, const v2* bp, const v2* bn, const int*, const int*, unsigned long long n_cells, hipStream_t s) {
    LF<kFiltCells, kFiltVecs, kFiltBlock>(ap, an, sp, sn, bp, bn, n_cells, s);
}
template <int CPL, int VECS, int BLOCK>
void LN(v2* ap, v2* an, int* sp, int* sn, const v2*, const v2*, const int* cp, const int* cn, unsigned long long n_cells, hipStream_t s) {
    const jg::Halves h = jg::halves_of(n_cells, CPL, (uint64_t)VECS * BLOCK);
    hipLaunchKernelGGL((jg::filt::k_merge_filtered<CPL, VECS, BLOCK, int>), dim3(2 * (unsigned)h.blocks), dim3(BLOCK), 0, s, (long long*)ap,
                       (long long*)an, sp, sn, cp, cn, h.n_units, h.tail, (unsigned)h.blocks);
}

int narrow_sweep(v2* AP, v2* AN, v2* BP, v2* BN, unsigned long long nv, int rounds) {
    const unsigned long long n_cells = nv * 2;
    hipStream_t s;
    CK(hipStreamCreate(&s));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    if (rounds > 500) rounds = 500;  // the generation stays below 2^16 (k_fill_f)
    int *SP, *SN, *CP, *CN;
    CK(hipMalloc(&SP, n_cells * 4)); CK(hipMalloc(&SN, n_cells * 4)); CK(hipMalloc(&CP, n_cells * 4)); CK(hipMalloc(&CN, n_cells * 4));
    unsigned* bad;  // [0] cells of A behind B, [1] cells whose shadow is not their clamp, [2] cells of B that do not fit
    CK(hipMalloc(&bad, 12));
    CK(hipMemsetAsync(bad, 0, 12, s));
    const unsigned g256 = (unsigned)((nv + 255) / 256), gc = (unsigned)((n_cells + 255) / 256);
    const std::vector<NVariant> vs = {
        {"parent (wide B, 2 cells B512)", LN_parent},
        {"narrow 2 cells U1 B256", LN<2, 1, 256>},
        {"narrow 2 cells U1 B512", LN<2, 1, 512>},
        {"narrow 2 cells U2 B256", LN<kNarrowCells, kNarrowVecs, kNarrowBlock>},  // the library's shape
        {"narrow 2 cells U4 B256", LN<2, 4, 256>},
        {"narrow 2 cells U2 B512", LN<2, 2, 512>},
        {"narrow 4 cells U1 B256", LN<4, 1, 256>},
        {"narrow 4 cells U1 B512", LN<4, 1, 512>},
        {"parent (again)", LN_parent},
    };
    const size_t nvar = vs.size();
    const auto clamp_all = [&] {
        hipLaunchKernelGGL(jg::filt::k_shadow_clamp, dim3(num_cus * 16), dim3(256), 0, s, (const long long*)AP, SP, 0ull, n_cells);
        hipLaunchKernelGGL(jg::filt::k_shadow_clamp, dim3(num_cus * 16), dim3(256), 0, s, (const long long*)AN, SN, 0ull, n_cells);
    };
    const auto codes = [&] {
        hipLaunchKernelGGL(k_codes, dim3(gc), dim3(256), 0, s, (const long long*)BP, CP, n_cells, bad + 2);
        hipLaunchKernelGGL(k_codes, dim3(gc), dim3(256), 0, s, (const long long*)BN, CN, n_cells, bad + 2);
    };
    const auto check = [&] {
        hipLaunchKernelGGL(k_count_behind, dim3(g256), dim3(256), 0, s, AP, AN, BP, BN, nv, bad);
        hipLaunchKernelGGL(k_count_shadow, dim3(gc), dim3(256), 0, s, (const long long*)AP, SP, n_cells, bad + 1);
        hipLaunchKernelGGL(k_count_shadow, dim3(gc), dim3(256), 0, s, (const long long*)AN, SN, n_cells, bad + 1);
    };
    const auto launch = [&](const NVariant& v) { v.launch(AP, AN, SP, SN, BP, BN, CP, CN, n_cells, s); };
    // the bench's data: A merged once, its shadow exact
    hipLaunchKernelGGL(k_synth, dim3(g256), dim3(256), 0, s, AP, AN, nv, 0u);
    hipLaunchKernelGGL(k_synth, dim3(g256), dim3(256), 0, s, BP, BN, nv, 2u);
    codes();
    clamp_all();
    launch(vs[0]);
    std::vector<std::vector<float>> t0(nvar), t1(nvar), t2(nvar);
    for (int r = -1; r < rounds; ++r)  // 0 %: 5 untimed launches, a fence, 20 launches between one event pair
        for (size_t k = 0; k < nvar; ++k) {
            for (int i = 0; i < 5; ++i) launch(vs[k]);
            CK(hipStreamSynchronize(s));
            CK(hipEventRecord(e0, s));
            for (int i = 0; i < 20; ++i) launch(vs[k]);
            CK(hipEventRecord(e1, s));
            CK(hipEventSynchronize(e1));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            if (r >= 0) t0[k].push_back(ms / 20);
            else check();
        }
    long long gen = 0;
    for (int pat = 1; pat <= 2; ++pat)
        for (int r = -1; r < rounds; ++r)
            for (size_t k = 0; k < nvar; ++k) {
                hipLaunchKernelGGL(k_fill_f, dim3(g256), dim3(256), 0, s, BP, BN, nv, pat, ++gen);
                codes();
                clamp_all();
                CK(hipEventRecord(e0, s));
                launch(vs[k]);
                CK(hipEventRecord(e1, s));
                CK(hipEventSynchronize(e1));
                float ms; CK(hipEventElapsedTime(&ms, e0, e1));
                if (r >= 0) (pat == 1 ? t1 : t2)[k].push_back(ms);
                else check();
            }
    std::printf("C2 shape: 10M keys x 64 replicas, int64, the bench's cells (A merged once); median of %d rounds, ms per launch\n", rounds);
    std::printf("%-32s %22s %22s %22s\n", "", "0 % (back to back)", "one column per key", "100 %");
    std::printf("%-32s %22s %22s %22s\n", "variant", "", "(behind a fill)", "(behind a fill)");
    for (size_t k = 0; k < nvar; ++k) std::printf("%-32s %22.3f %22.3f %22.3f\n", vs[k].name, median(t0[k]), median(t1[k]), median(t2[k]));
    std::printf("%-32s %22.3f %22.3f %22.3f\n", "A/A spread (parent twice)", std::fabs(median(t0[0]) - median(t0[nvar - 1])),
                std::fabs(median(t1[0]) - median(t1[nvar - 1])), std::fabs(median(t2[0]) - median(t2[nvar - 1])));
    for (size_t k = 0; k < nvar; ++k)
        std::printf("%-32s %10.3f .. %-10.3f %10.3f .. %-10.3f %10.3f .. %-10.3f (min .. max of rounds)\n", vs[k].name,
                    *std::min_element(t0[k].begin(), t0[k].end()), *std::max_element(t0[k].begin(), t0[k].end()),
                    *std::min_element(t1[k].begin(), t1[k].end()), *std::max_element(t1[k].begin(), t1[k].end()),
                    *std::min_element(t2[k].begin(), t2[k].end()), *std::max_element(t2[k].begin(), t2[k].end()));
    unsigned h[3] = {0, 0, 0};
    CK(hipMemcpy(h, bad, 12, hipMemcpyDeviceToHost));
    const bool ok = h[0] == 0 && h[1] == 0 && h[2] == 0;
    std::printf("vectors of A left behind B over every variant and pattern: %u; cells whose shadow is not their clamp: %u; cells of B that do not fit: %u%s\n",
                h[0], h[1], h[2], ok ? " (ok)" : " (WRONG)");
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
    if (argc > 2 && std::string(argv[2]) == "filter") return filter_sweep(AP, AN, BP, BN, nv, std::atoi(argv[1]) > 0 ? std::atoi(argv[1]) : 7);
    if (argc > 2 && std::string(argv[2]) == "narrow") return narrow_sweep(AP, AN, BP, BN, nv, std::atoi(argv[1]) > 0 ? std::atoi(argv[1]) : 7);
    if (argc > 2 && std::string(argv[2]) == "steady") return steady_sweep(AP, AN, BP, BN, nv, std::atoi(argv[1]) > 0 ? std::atoi(argv[1]) : 7);
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
