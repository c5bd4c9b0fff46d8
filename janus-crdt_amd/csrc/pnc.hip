// pnc.hip — PN-Counter store and kernels (gfx950, wave64, no MFMA: integer bandwidth work).
//
// Layout in HBM: P and N are row-major [n_keys x R] arrays of the store's width (int32 = the
// reference's `int`, int64 = the BASELINE variant).  Row = interned key, column = interned replica.
//
// Kernels and their roofline (HBM):
//   k_merge_dense    A = max(A, B) over identity rows.  Reads A.P A.N B.P B.N: 4 x elem_bytes per cell
//                    (32 B at int64), and writes back only the 128-B lines of A.P / A.N that a cell of B
//                    raised: up to 2 x elem_bytes more (48 B per cell when every line changes, 32 B for a
//                    re-delivered batch).  Two halves of one grid: P's workgroups, then N's (two read streams
//                    at a time); kDenseVecs 16-B vectors of A and of B per lane, non-temporal.  This is
//                    PNCounter.Merge (PNCounters.cs:131-144).
//   k_merge_filtered (pnc_filter_kernels.hpp) the same merge of an int64 store by its 32-bit shadow sP / sN = clamp32(P / N):
//                    reads sA.P sA.N B.P B.N, 24 B per cell, and A itself only for lines that hold a cell at a clamp
//                    value; writes the raised lines of A with their 64 B of shadow.  From the third consecutive dense
//                    identity merge on (merge_dense_store: cold -> armed -> valid; k_merge_build writes the shadow
//                    at the second); every other writer of P / N takes them through jg_pnc::rw_P / rw_N, which
//                    drops the shadow.
//   the narrow form  an int64 identity batch (jg_rows) whose every cell is ABSENT or fits 32 bits is held as 4-byte codes
//                    (pnc_filter.hpp `narrow`), decided where the batch is born: jg_rows_upload narrows each landed chunk
//                    under the next chunk's copy (k_rows_narrow), jg_synth_pnc_rows writes the codes.  The three dense
//                    kernels read it in place and widen in registers (k_merge_dense_narrow, k_merge_build / k_merge_filtered
//                    with BT = int): a steady launch reads sA and B at 4 B each, 16 B per cell (P and N), the first launch
//                    and the build launch 8 B less per cell than with a wide batch.  Every other reader goes through
//                    jg::rows_wide, which widens the batch in place first.
//   k_merge_indexed  scatter-max of received rows into their keys (atomicMax: rows may repeat a
//                    key inside one committed batch, SafeCRDTManager.cs:122-146).
//   k_apply_ops      Increment/Decrement (PNCounters.cs:97-112): wrapping atomic adds.
//   k_values         PNCounter.Get (PNCounters.cs:87-90): one wave per key, exact prefix sums in
//                    column order to reproduce the checked LINQ Sum's OverflowException.
//   k_restride       jg_pnc_reserve's widening: dst[k][0..R_old) = src[k][0..R_old), zero elsewhere (a row
//                    the Dictionary<Guid,int> grows into, PNCounters.cs:131-144).  Reads the old bytes once,
//                    writes the new bytes once: (old + new) bytes at HBM rate.
#include <algorithm>
#include <cstdlib>

#include "launch.hpp"
#include "pnc_filter_kernels.hpp"

namespace {

constexpr int kBlock = 256;

struct I64x2 { long long x, y; };
struct I32x4 { int x, y, z, w; };

template <int EB> __device__ __forceinline__ uint4 vmax(uint4 a, uint4 b);
template <> __device__ __forceinline__ uint4 vmax<8>(uint4 a, uint4 b) {
    I64x2 p = __builtin_bit_cast(I64x2, a), q = __builtin_bit_cast(I64x2, b);
    I64x2 r{p.x > q.x ? p.x : q.x, p.y > q.y ? p.y : q.y};
    return __builtin_bit_cast(uint4, r);
}
template <> __device__ __forceinline__ uint4 vmax<4>(uint4 a, uint4 b) {
    I32x4 p = __builtin_bit_cast(I32x4, a), q = __builtin_bit_cast(I32x4, b);
    I32x4 r{max(p.x, q.x), max(p.y, q.y), max(p.z, q.z), max(p.w, q.w)};
    return __builtin_bit_cast(uint4, r);
}

typedef unsigned int v4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 nt_load(const uint4* p) {
    return __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const v4u*>(p)));
}
__device__ __forceinline__ void nt_store(uint4* p, uint4 v) {
    __builtin_nontemporal_store(__builtin_bit_cast(v4u, v), reinterpret_cast<v4u*>(p));
}

template <int EB> struct Elem;
template <> struct Elem<4> { using T = int; };
template <> struct Elem<8> { using T = long long; };

// True where the two vectors differ in any bit.
__device__ __forceinline__ bool differs(uint4 a, uint4 b) { return ((a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w)) != 0; }

// Store elision (merge kernels): max is idempotent and most merges are no-ops for most cells (a replica advances
// its own column only, every message is a full state, anti-entropy re-delivers merged states), so a vector of A
// is stored only if its aligned group of kElideLanes lanes holds a lane whose maximum differs from what it loaded:
// 8 lanes x 16 B = one 128-B line where the lanes' vectors are consecutive and the group's first is line-aligned
// (k_merge_dense always; k_merge_grouped where the row is a multiple of 128 B), so a line is written whole or
// not at all.  Granularity measured against per-lane (16 B) and per-wave (1 KB) elision over 0 - 100 % changed
// cells (tools/tune_pnc.hip, profiles/r07/tune_pnc_elide.txt).  Correctness rests on neither grouping nor
// alignment: a lane that stores writes the maximum, a lane that skips held an unchanged value.  `mask` is the
// wave's ballot of changed lanes (inactive lanes read as unchanged).
constexpr uint32_t kElideLanes = 8;
__device__ __forceinline__ bool group_changed(unsigned long long mask, uint32_t lane) {
    return ((mask >> (lane & (64 - kElideLanes))) & ((1u << kElideLanes) - 1)) != 0;
}

// Dense merge: nv 16-byte vectors per array plus `tail` trailing cells (< 16 B) done by block 0.  The grid is two
// halves of `half` workgroups: the first merges P (A.P, B.P), the second N (A.N, B.N), so in dispatch order the chip
// streams two arrays at a time, then the other two, instead of four at once.  A workgroup takes kDenseVecs vectors
// per lane, kDenseBlock apart (a wave-instruction reads 1 KB contiguous, an aligned group of kElideLanes lanes is one
// 128-B line), every load issued before the first use.  Measured on MI355X in the regime the kernel now mostly
// runs in — four read streams, nothing stored — and behind batches that raise one column per key or every cell
// (tools/tune_pnc.hip `steady`, profiles/r08/tune_pnc_steady*.txt), against the four-streams-per-workgroup shape it
// had since round 1 and against 2 / 4 vectors per lane, workgroups of 512 / 1024, bounded grids (grid-stride and
// block-chunk walks), P then N inside a workgroup, default-policy loads and LDS-DMA loads: see DESIGN.md §4 for
// what each measured.  P and N are elided separately as before (each half writes only its own array); the bounds
// test is a predicate, not a branch around the ballot, so every lane of a wave that loaded data votes (lanes past
// nv vote unchanged).
constexpr int kDenseVecs = 1;     // 16-B vectors of each array per lane
constexpr int kDenseBlock = 256;  // lanes per workgroup: kDenseVecs x kDenseBlock vectors per workgroup

// Vector i of the batch beside A's 16-B vector i.  BV = uint4: the batch's own cells (the wide form, and every int32
// batch).  BV = uint2 (int64 stores only): two 4-byte codes of a narrow batch (jg_rows), widened in registers.
__device__ __forceinline__ uint4 ld_batch_vec(const uint4* B, uint64_t i) { return nt_load(B + i); }
__device__ __forceinline__ uint4 ld_batch_vec(const uint2* B, uint64_t i) {
    const jg::filt::v2i c = __builtin_nontemporal_load(reinterpret_cast<const jg::filt::v2i*>(B) + i);
    return __builtin_bit_cast(uint4, I64x2{jg::filt::widen(c.x), jg::filt::widen(c.y)});
}
template <class T> __device__ __forceinline__ T ld_batch_cell(const uint4* B, uint64_t nv, uint32_t k) { return reinterpret_cast<const T*>(B + nv)[k]; }
template <class T> __device__ __forceinline__ T ld_batch_cell(const uint2* B, uint64_t nv, uint32_t k) {
    return (T)jg::filt::widen(reinterpret_cast<const int*>(B + nv)[k]);
}

template <int EB, class BV>
__device__ __forceinline__ void merge_dense_body(uint4* __restrict__ AP, uint4* __restrict__ AN, const BV* __restrict__ BP,
                                                 const BV* __restrict__ BN, uint64_t nv, uint32_t tail, uint32_t half) {
    using T = typename Elem<EB>::T;
    static_assert(sizeof(BV) == 16 || EB == 8, "the narrow form is an int64 batch's");
    const bool isN = blockIdx.x >= half;
    uint4* const A = isN ? AN : AP;
    const BV* const B = isN ? BN : BP;
    const uint64_t base = (uint64_t)(blockIdx.x - (isN ? half : 0)) * (kDenseVecs * kDenseBlock) + threadIdx.x;
    uint4 a[kDenseVecs], b[kDenseVecs];
    bool in[kDenseVecs];
#pragma unroll
    for (int u = 0; u < kDenseVecs; ++u) {
        const uint64_t i = base + u * kDenseBlock;
        in[u] = i < nv;
        a[u] = b[u] = uint4{};
        if (in[u]) a[u] = nt_load(A + i), b[u] = ld_batch_vec(B, i);
    }
    const uint32_t lane = threadIdx.x & 63;
#pragma unroll
    for (int u = 0; u < kDenseVecs; ++u) {
        const uint4 m = vmax<EB>(a[u], b[u]);
        const unsigned long long c = __ballot(in[u] && differs(m, a[u]));
        if (in[u] && group_changed(c, lane)) nt_store(A + base + u * kDenseBlock, m);
    }
    if (blockIdx.x == 0 && threadIdx.x < tail) {
        T* ap = reinterpret_cast<T*>(AP + nv) + threadIdx.x;
        T* an = reinterpret_cast<T*>(AN + nv) + threadIdx.x;
        const T bp = ld_batch_cell<T>(BP, nv, threadIdx.x);
        const T bn = ld_batch_cell<T>(BN, nv, threadIdx.x);
        if (bp > *ap) *ap = bp;
        if (bn > *an) *an = bn;
    }
}

template <int EB>
__global__ __launch_bounds__(kDenseBlock) void k_merge_dense(uint4* __restrict__ AP, uint4* __restrict__ AN,
                                                             const uint4* __restrict__ BP, const uint4* __restrict__ BN,
                                                             uint64_t nv, uint32_t tail, uint32_t half) {
    merge_dense_body<EB, uint4>(AP, AN, BP, BN, nv, tail, half);
}

// The same merge of an int64 store with a narrow batch: nv 16-B vectors of A beside nv 8-B vectors of codes.
__global__ __launch_bounds__(kDenseBlock) void k_merge_dense_narrow(uint4* __restrict__ AP, uint4* __restrict__ AN,
                                                                    const uint2* __restrict__ BP, const uint2* __restrict__ BN,
                                                                    uint64_t nv, uint32_t tail, uint32_t half) {
    merge_dense_body<8, uint2>(AP, AN, BP, BN, nv, tail, half);
}

// Scatter-max: cell (m, c) of the received rows into row keys[m].  ABSENT cells are skipped.
template <int EB>
__global__ __launch_bounds__(kBlock) void k_merge_indexed(typename Elem<EB>::T* __restrict__ AP, typename Elem<EB>::T* __restrict__ AN,
                                                          const typename Elem<EB>::T* __restrict__ BP,
                                                          const typename Elem<EB>::T* __restrict__ BN,
                                                          const uint32_t* __restrict__ keys, uint64_t n_rows, uint32_t R) {
    using T = typename Elem<EB>::T;
    const T absent = EB == 4 ? (T)INT32_MIN : (T)INT64_MIN;
    const uint64_t n = n_rows * R;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const uint64_t m = i / R, c = i - m * R;
        const uint64_t at = (uint64_t)keys[m] * R + c;
        const T p = BP[i], q = BN[i];
        if (p != absent) atomicMax(AP + at, p);
        if (q != absent) atomicMax(AN + at, q);
    }
}

// The same scatter-max with one wave per received row (lanes over columns): no 64-bit division per
// cell, coalesced row loads and row-contiguous atomics.  Used when a row fills most of a wave (R >= 32).
template <int EB>
__global__ __launch_bounds__(kBlock) void k_merge_indexed_rows(typename Elem<EB>::T* __restrict__ AP, typename Elem<EB>::T* __restrict__ AN,
                                                               const typename Elem<EB>::T* __restrict__ BP,
                                                               const typename Elem<EB>::T* __restrict__ BN,
                                                               const uint32_t* __restrict__ keys, uint64_t n_rows, uint32_t R) {
    using T = typename Elem<EB>::T;
    const T absent = EB == 4 ? (T)INT32_MIN : (T)INT64_MIN;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t n_waves = ((uint64_t)gridDim.x * kBlock) >> 6;
    for (uint64_t m = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6; m < n_rows; m += n_waves) {
        const uint64_t at = (uint64_t)keys[m] * R, src = m * R;
        for (uint32_t c = lane; c < R; c += 64) {
            const T p = BP[src + c], q = BN[src + c];
            if (p != absent) atomicMax(AP + at + c, p);
            if (q != absent) atomicMax(AN + at + c, q);
        }
    }
}

// Duplicate-aware scatter-max with no atomics on the data, two passes over the batch's keys (a committed
// wave folds several states of one key, SafeCRDTManager.cs:122-146).  Pass 1 (k_group_link) links each
// key's rows into a list: next[m] = the key's previous head, head[key] = gen << 32 | m (one atomicExch per
// row).  Pass 2 (k_merge_grouped): the head row of every key loads its A row once, max-folds every B row of
// the key in registers — each B row's load issued together with its next[] link, so a key held k times
// costs k - 1 dependent hops — and stores the 128-B lines of A that the fold raised, once (store elision, above:
// a key whose rows are all at or below A writes nothing); the other rows of the key do nothing.  Heads carry the
// batch's generation: a head left by an earlier batch reads as empty, so nothing resets them (the list
// head's `head[key] = kNil` store was one more random write per distinct key: 0.578 -> 0.566 ms per 1M rows,
// tools/tune_grouped.hip).  Atomics ran at ~1.3 TB/s of added bytes on MI355X against ~6 TB/s for plain
// stores (MI355X_MICROARCH.md, atomics table), and random 4-B atomics ~17x slower again: a per-cell
// atomicMax for repeated keys (39 % of the rows of a uniform batch of n rows over 2n keys) and an
// occurrence count per row both measured slower (tools/tune_grouped.hip).  ABSENT (the
// width's minimum) needs no test: max(a, ABSENT) = a.
constexpr uint32_t kNil = 0xFFFFFFFFu;

__global__ __launch_bounds__(kBlock) void k_group_link(const uint32_t* __restrict__ keys, uint64_t n, unsigned long long* __restrict__ head,
                                                       uint32_t* __restrict__ next, unsigned long long gen) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const unsigned long long old = atomicExch(head + keys[i], gen << 32 | i);
        next[i] = (old >> 32) == gen ? (uint32_t)old : kNil;
    }
}

// One wave per received row, U rows in flight; the row (R x EB bytes) is a whole number of 16-B vectors
// and each lane owns the same vector slot(s) of every row it touches.
template <int EB, int U>
__global__ __launch_bounds__(kBlock) void k_merge_grouped(typename Elem<EB>::T* __restrict__ AP, typename Elem<EB>::T* __restrict__ AN,
                                                          const typename Elem<EB>::T* __restrict__ BP,
                                                          const typename Elem<EB>::T* __restrict__ BN, const uint32_t* __restrict__ keys,
                                                          const unsigned long long* __restrict__ head, const uint32_t* __restrict__ next,
                                                          uint64_t n_rows, uint32_t R, unsigned long long gen) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t nv = R * EB / 16;  // vectors per array row
    const uint64_t n_waves = ((uint64_t)gridDim.x * kBlock) >> 6;
    for (uint64_t m0 = (((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6) * U; m0 < n_rows; m0 += n_waves * U) {
        uint64_t key[U];
        bool lead[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t m = m0 + u;
            key[u] = m < n_rows ? keys[m] : 0;
            lead[u] = m < n_rows && head[key[u]] == (gen << 32 | m);
        }
        for (uint32_t v = lane; v < 2 * nv; v += 64) {
            const bool isP = v < nv;
            const uint32_t w = isP ? v : v - nv;
            const auto* B = isP ? BP : BN;
            auto* A = isP ? AP : AN;
            uint4 a[U], a0[U], b[U];  // a0: the A vector as loaded (store elision)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (lead[u]) {
                    b[u] = nt_load(reinterpret_cast<const uint4*>(B + (m0 + u) * R) + w);
                    a0[u] = *(reinterpret_cast<const uint4*>(A + key[u] * R) + w);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!lead[u]) continue;
                a[u] = vmax<EB>(a0[u], b[u]);
                uint64_t hops = 0;  // a list holds at most n_rows - 1 more rows: a bound every walk reaches
                for (uint32_t cur = next[m0 + u]; cur != kNil && ++hops < n_rows;) {  // the key's other rows
                    const uint4 bb = nt_load(reinterpret_cast<const uint4*>(B + (uint64_t)cur * R) + w);
                    const uint32_t nx = next[cur];
                    a[u] = vmax<EB>(a[u], bb);
                    cur = nx;
                }
                // lead[u] and the list walk are wave-uniform: the ballot is taken by the lanes of this trip of the
                // v loop (the last trip's idle lanes vote unchanged)
                if (group_changed(__ballot(differs(a[u], a0[u])), lane)) *(reinterpret_cast<uint4*>(A + key[u] * R) + w) = a[u];
            }
        }
    }
}

// Row copy (write: keys on the destination side; read: keys on the source side).
template <int EB>
__global__ __launch_bounds__(kBlock) void k_rows_copy(typename Elem<EB>::T* __restrict__ dst, const typename Elem<EB>::T* __restrict__ src,
                                                      const uint32_t* __restrict__ keys, uint64_t n_rows, uint32_t R, int scatter) {
    const uint64_t n = n_rows * R;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const uint64_t m = i / R, c = i - m * R;
        const uint64_t at = (uint64_t)keys[m] * R + c;
        if (scatter) dst[at] = src[i];
        else dst[i] = src[at];
    }
}

// Increment / Decrement: unchecked '+=' == wrapping add; order-free, so atomics are exact.
template <int EB>
__global__ __launch_bounds__(kBlock) void k_apply_ops(typename Elem<EB>::T* __restrict__ P, typename Elem<EB>::T* __restrict__ N,
                                                      const uint32_t* __restrict__ key, const uint32_t* __restrict__ col,
                                                      const long long* __restrict__ delta, const uint8_t* __restrict__ is_n,
                                                      uint64_t n_ops, uint32_t R) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n_ops; i += (uint64_t)gridDim.x * kBlock) {
        const uint64_t at = (uint64_t)key[i] * R + col[i];
        auto* base = is_n[i] ? N : P;
        if constexpr (EB == 4) atomicAdd(reinterpret_cast<unsigned int*>(base + at), (unsigned int)delta[i]);
        else atomicAdd(reinterpret_cast<unsigned long long*>(base + at), (unsigned long long)delta[i]);
    }
}

// ---- PNCounter.Get: checked Sum in column order -------------------------------------------------
template <int EB> struct Acc;
template <> struct Acc<4> { using T = long long; };  // 64 x 2^31 fits easily
template <> struct Acc<8> { using T = __int128; };   // exact for any 64-bit prefix

__device__ __forceinline__ long long shfl_up_acc(long long v, int d) { return __shfl_up(v, d, 64); }
__device__ __forceinline__ __int128 shfl_up_acc(__int128 v, int d) {
    long long lo = (long long)v, hi = (long long)(v >> 64);
    lo = __shfl_up(lo, d, 64);
    hi = __shfl_up(hi, d, 64);
    return ((__int128)hi << 64) | (unsigned long long)lo;
}
__device__ __forceinline__ long long shfl_acc(long long v, int src) { return __shfl(v, src, 64); }
__device__ __forceinline__ __int128 shfl_acc(__int128 v, int src) {
    long long lo = (long long)v, hi = (long long)(v >> 64);
    lo = __shfl(lo, src, 64);
    hi = __shfl(hi, src, 64);
    return ((__int128)hi << 64) | (unsigned long long)lo;
}

// Returns the exact sum of row[0..R); sets `of` if any prefix leaves T's range.
template <int EB>
__device__ __forceinline__ typename Acc<EB>::T checked_row_sum(const typename Elem<EB>::T* row, uint32_t R, int lane, bool& of) {
    using T = typename Elem<EB>::T;
    using A = typename Acc<EB>::T;
    const A lo = EB == 4 ? (A)INT32_MIN : (A)INT64_MIN;
    const A hi = EB == 4 ? (A)INT32_MAX : (A)INT64_MAX;
    A carry = 0;
    for (uint32_t c0 = 0; c0 < R; c0 += 64) {
        A x = (c0 + lane < R) ? (A)row[c0 + lane] : (A)0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            A y = shfl_up_acc(x, d);
            if (lane >= d) x += y;
        }
        const A pre = carry + x;
        of |= __any(pre < lo || pre > hi) != 0;
        carry = shfl_acc(pre, 63);
    }
    (void)sizeof(T);
    return carry;
}

// at / count / of_code serve the reads by key name (query.hip): answer q goes to slot at[q] (NULL: q), only the
// first *count keys of the list are answered (NULL: all n; the list was appended to by the launch before, so its
// length never visits the host), and an overflow is reported as of_code (jg_pnc_values: 1).
template <int EB>
__global__ __launch_bounds__(kBlock) void k_values(const typename Elem<EB>::T* __restrict__ P, const typename Elem<EB>::T* __restrict__ N,
                                                   uint32_t R, const uint32_t* __restrict__ keys, uint64_t n,
                                                   long long* __restrict__ out, uint8_t* __restrict__ ovf,
                                                   const uint32_t* __restrict__ at, const unsigned long long* __restrict__ count,
                                                   uint8_t of_code) {
    using T = typename Elem<EB>::T;
    using UT = std::make_unsigned_t<T>;
    const int lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * kBlock) >> 6;
    if (count && *count < n) n = *count;
    for (uint64_t q = wave; q < n; q += n_waves) {
        const uint64_t k = keys ? keys[q] : q;
        bool of = false;
        const auto sp = checked_row_sum<EB>(P + k * R, R, lane, of);
        const auto sn = checked_row_sum<EB>(N + k * R, R, lane, of);
        if (lane == 0) {
            // ΣP and ΣN are in range when !of; '-' is unchecked: wrap at the width.
            const T v = (T)((UT)(T)sp - (UT)(T)sn);
            const uint64_t o = at ? at[q] : q;
            out[o] = of ? 0 : (long long)v;
            ovf[o] = of ? of_code : 0;
        }
    }
}

// Re-stride copy (jg_pnc_reserve): the destination is n_units units (16-B vectors where both row sizes are whole
// vectors, else cells) in rows of `dw`; unit (row, col) takes the source's (row, col) where row < src_rows and
// col < sw, zero elsewhere, so every destination unit is written exactly once and no memset runs ahead of the
// copy.  One unit per lane over a flat grid, as k_merge_dense: measured on MI355X on the widen's P array (1M keys,
// 64 -> 128 int64 columns, 1.6 GB moved; tools/tune_reserve.hip) at 0.259 ms = 6.2 TB/s against 0.297 ms for a
// device copy of the old bytes plus a memset of the new ones; 2 / 4 / 8 units in flight per lane 0.265 / 0.289 /
// 0.283 ms, a grid capped at 16 blocks per CU 0.292 ms (4 units per lane: 0.308), plain instead of non-temporal
// accesses the same (0.257);
// past kRestrideBlocks blocks the grid strides.  Stores are coalesced, loads contiguous inside a row.  Index
// arithmetic: the block's first (row, col) comes from one 32-bit divide up front and moves by the grid's step
// (step_rows, step_cols: divided on the host) with a compare; a lane's own unit lies at most kBlock / dw + 1 rows
// further, found by a float reciprocal with a +-1 fix-up (exact: the quotient is at most 257 and dw < 2^30) — no
// 64-bit divide per unit.  Touched once: non-temporal both ways, no LDS.
template <class T> __device__ __forceinline__ T nt_ld(const T* p) { return __builtin_nontemporal_load(p); }
template <> __device__ __forceinline__ uint4 nt_ld<uint4>(const uint4* p) { return nt_load(p); }
template <class T> __device__ __forceinline__ void nt_st(T* p, T v) { __builtin_nontemporal_store(v, p); }
template <> __device__ __forceinline__ void nt_st<uint4>(uint4* p, uint4 v) { nt_store(p, v); }

constexpr uint64_t kRestrideBlocks = 1u << 16;  // x kBlock = 16.8M units a pass (268 MB of vectors)

template <class T>
__global__ __launch_bounds__(kBlock) void k_restride(T* __restrict__ dst, const T* __restrict__ src, uint32_t sw, uint32_t dw, float rdw,
                                                     uint64_t src_rows, uint64_t n_units, uint64_t step_rows, uint32_t step_cols) {
    const uint32_t first = blockIdx.x * kBlock;  // < 2^24 (kRestrideBlocks)
    uint64_t row0 = first / dw;
    uint32_t col0 = first - (uint32_t)row0 * dw;
    for (uint64_t base = first; base < n_units; base += (uint64_t)gridDim.x * kBlock) {
        const uint64_t i = base + threadIdx.x;
        if (i < n_units) {
            const uint32_t c = col0 + threadIdx.x;  // < dw + kBlock
            uint32_t q = (uint32_t)((float)c * rdw);
            uint32_t col = c - q * dw;
            if ((int32_t)col < 0) --q, col += dw;
            else if (col >= dw) ++q, col -= dw;
            const uint64_t row = row0 + q;
            T v{};
            if (row < src_rows && col < sw) v = nt_ld(src + row * sw + col);
            nt_st(dst + i, v);
        }
        row0 += step_rows;
        col0 += step_cols;
        if (col0 >= dw) col0 -= dw, ++row0;
    }
}

void check_store(const jg_pnc* p, const char* fn) {
    JG_REQUIRE(p, JG_EINVAL, "%s: store is NULL", fn);
}

void check_keys(const uint32_t* k, uint64_t n, uint64_t n_keys, const char* fn) {
    for (uint64_t i = 0; i < n; ++i)
        JG_REQUIRE(k[i] < n_keys, JG_EINVAL, "%s: key_idx[%llu] = %u out of range (n_keys %llu)", fn,
                   (unsigned long long)i, k[i], (unsigned long long)n_keys);
}

// Upload key indices (validated) to ctx scratch.
uint32_t* upload_keys(jg_ctx* ctx, const uint32_t* key_idx, uint64_t n, uint64_t n_keys, const char* fn) {
    check_keys(key_idx, n, n_keys, fn);
    auto* d = static_cast<uint32_t*>(jg::scratch(ctx, ctx->scratch, n * 4));
    JG_HIP(hipMemcpyAsync(d, key_idx, n * 4, hipMemcpyHostToDevice, ctx->stream));
    return d;
}

// narrow: B is an int64 batch's 4-byte codes (eb == 8 only).
void launch_merge_dense(jg_ctx* ctx, uint32_t eb, void* AP, void* AN, const void* BP, const void* BN, uint64_t n_cells, bool narrow = false) {
    const uint64_t bytes = n_cells * eb;
    const uint64_t nv = bytes / 16;
    const uint32_t tail = (uint32_t)((bytes - nv * 16) / eb);
    constexpr uint64_t per = (uint64_t)kDenseVecs * kDenseBlock;
    const uint64_t blocks = (nv + per - 1) / per;  // per array: the grid holds P's, then N's
    JG_REQUIRE(2 * blocks < 0xFFFFFFFFull, JG_EINVAL, "merge: %llu cells exceed one launch", (unsigned long long)n_cells);
    const unsigned half = blocks ? (unsigned)blocks : 1u;  // block 0 exists for the trailing cells
    if (narrow) {
        hipLaunchKernelGGL(k_merge_dense_narrow, dim3(2 * half), dim3(kDenseBlock), 0, ctx->stream, (uint4*)AP, (uint4*)AN, (const uint2*)BP,
                           (const uint2*)BN, nv, tail, half);
    } else {
        jg::dispatch_eb(eb, [&](auto EB) {
            hipLaunchKernelGGL(k_merge_dense<EB()>, dim3(2 * half), dim3(kDenseBlock), 0, ctx->stream, (uint4*)AP, (uint4*)AN, (const uint4*)BP,
                               (const uint4*)BN, nv, tail, half);
        });
    }
    JG_HIP(hipGetLastError());
}

// ---- the dense merge by the 32-bit shadow (int64 stores; pnc_filter_kernels.hpp) -------------------
// The filtered kernel's shape: kFiltCells cells per lane and unit (2: an 8-B shadow load beside one 16-B vector of B,
// 8 lanes to a 128-B line of A; 4: a 16-B shadow load beside two vectors of B, 4 lanes to a line), kFiltVecs units per
// lane, kFiltBlock lanes per workgroup.  Measured against the other shapes in tools/tune_pnc.hip `filter`
// (profiles/r09/tune_pnc_filter.txt): every shape reads a merged batch in 2.23 - 2.28 ms against k_merge_dense's
// 2.88 ms; the 4-cell shapes are the fastest there by 0.02 ms but 0.4 ms slower than k_merge_dense when every line
// changes (4 lanes store a 128-B line of A in two instructions each); of the 2-cell shapes this one is at or ahead of
// k_merge_dense on all three patterns and the fastest on the merged batch.
constexpr int kFiltCells = 2;
constexpr int kFiltVecs = 1;
constexpr int kFiltBlock = 512;
constexpr int kBuildBlock = 256;

unsigned halves_for(uint64_t n_units, uint64_t per, uint64_t n_cells) {
    const uint64_t blocks = (n_units + per - 1) / per;  // per array: the grid holds P's, then N's
    JG_REQUIRE(2 * blocks < 0xFFFFFFFFull, JG_EINVAL, "merge: %llu cells exceed one launch", (unsigned long long)n_cells);
    return blocks ? (unsigned)blocks : 1u;  // a half's first block exists for the trailing cells
}

template <int CELLS, int VECS, int BLOCK, class BT>
void launch_merge_filtered_as(jg_pnc* p, const void* BP, const void* BN, uint64_t n_cells) {
    const uint64_t n_units = n_cells / CELLS;
    const uint32_t tail = (uint32_t)(n_cells - n_units * CELLS);
    const unsigned half = halves_for(n_units, (uint64_t)VECS * BLOCK, n_cells);
    hipLaunchKernelGGL((jg::filt::k_merge_filtered<CELLS, VECS, BLOCK, BT>), dim3(2 * half), dim3(BLOCK), 0, p->ctx->stream,
                       p->P_.as<long long>(), p->N_.as<long long>(), p->sP.as<int>(), p->sN.as<int>(), (const BT*)BP, (const BT*)BN, n_units,
                       tail, half);
    JG_HIP(hipGetLastError());
}

// The filtered kernel's shape for a narrow batch (4-byte codes of B beside the 4-byte shadow: two equal read streams),
// chosen like the wide batch's in tools/tune_pnc.hip `narrow`.
constexpr int kNarrowCells = 2;
constexpr int kNarrowVecs = 2;
constexpr int kNarrowBlock = 256;

void launch_merge_filtered(jg_pnc* p, const void* BP, const void* BN, uint64_t n_cells, bool narrow) {
    if (narrow) launch_merge_filtered_as<kNarrowCells, kNarrowVecs, kNarrowBlock, int>(p, BP, BN, n_cells);
    else launch_merge_filtered_as<kFiltCells, kFiltVecs, kFiltBlock, long long>(p, BP, BN, n_cells);
}

template <class BT> void launch_build_as(jg_pnc* p, const void* BP, const void* BN, uint64_t n_units, uint32_t tail, unsigned half) {
    hipLaunchKernelGGL((jg::filt::k_merge_build<kBuildBlock, BT>), dim3(2 * half), dim3(kBuildBlock), 0, p->ctx->stream, p->P_.as<long long>(),
                       p->N_.as<long long>(), p->sP.as<int>(), p->sN.as<int>(), (const BT*)BP, (const BT*)BN, n_units, tail, half);
}

// The build launch over the batch's cells, then the clamp pass over the store's cells behind the batch.
void launch_merge_build(jg_pnc* p, const void* BP, const void* BN, uint64_t n_cells, bool narrow) {
    jg_ctx* ctx = p->ctx;
    const uint64_t n_units = n_cells / 2;
    const uint32_t tail = (uint32_t)(n_cells - n_units * 2);
    const unsigned half = halves_for(n_units, kBuildBlock, n_cells);
    if (narrow) launch_build_as<int>(p, BP, BN, n_units, tail, half);
    else launch_build_as<long long>(p, BP, BN, n_units, tail, half);
    const uint64_t all = p->n_keys * p->R;
    if (n_cells < all) {
        const unsigned g = jg::grid_for(ctx, all - n_cells, 256, 16);
        hipLaunchKernelGGL(jg::filt::k_shadow_clamp, dim3(g), dim3(256), 0, ctx->stream, p->P_.as<long long>(), p->sP.as<int>(), n_cells, all);
        hipLaunchKernelGGL(jg::filt::k_shadow_clamp, dim3(g), dim3(256), 0, ctx->stream, p->N_.as<long long>(), p->sN.as<int>(), n_cells, all);
    }
    JG_HIP(hipGetLastError());
}

// The shadow's buffers for the store's shape (kept across cold spells).  false: no room on the device; remembered
// until the shape changes (pnc_grow), so a store that does not fit does not ask the allocator on every merge.
bool shadow_ready(jg_pnc* p) {
    const size_t bytes = (size_t)p->n_keys * p->R * 4;
    if (p->sP.p && p->sN.p && p->sP.bytes >= bytes && p->sN.bytes >= bytes) return true;
    if (p->filt_nomem) return false;
    try {
        p->sP.alloc(bytes);
        p->sN.alloc(bytes);
    } catch (const jg::Error&) {
        p->sP.release();
        p->sN.release();
        p->filt_nomem = true;
        (void)hipGetLastError();  // the failed allocation's code must not surface at the next launch check
        jg::clear_error();
        return false;
    }
    return true;
}

void drop_shadow(jg_pnc* p) {
    p->sP.release();
    p->sN.release();
    p->filt = jg_pnc::kFiltCold;
    p->filt_nomem = false;
}

// A dense identity merge of n_rows rows into the store: the one writer that does not go through rw_P / rw_N.
// int32 stores and stores with the filter off run k_merge_dense and stay cold.  An int64 store runs it while cold
// (and becomes armed: nothing else has written since this merge), the build launch while armed (and becomes valid),
// the filtered kernel while valid.  narrow: the batch's form (jg_rows; int64 stores only): every one of the three
// kernels reads a narrow batch as 4-byte codes.
void merge_dense_store(jg_pnc* p, const void* BP, const void* BN, uint64_t n_rows, bool narrow = false) {
    jg_ctx* ctx = p->ctx;
    const uint64_t n_cells = n_rows * p->R;
    if (p->eb == 8 && p->filt_on) {
        if (p->filt == jg_pnc::kFiltValid) return launch_merge_filtered(p, BP, BN, n_cells, narrow);
        if (p->filt == jg_pnc::kFiltArmed && shadow_ready(p)) {
            launch_merge_build(p, BP, BN, n_cells, narrow);
            p->filt = jg_pnc::kFiltValid;
            return;
        }
        launch_merge_dense(ctx, 8, p->P_.p, p->N_.p, BP, BN, n_cells, narrow);
        p->filt = jg_pnc::kFiltArmed;
        return;
    }
    launch_merge_dense(ctx, p->eb, p->rw_P(), p->rw_N(), BP, BN, n_cells, narrow);
}

// The store's per-key list heads (generation-tagged) and a next[] link per received row (grown to the
// largest batch); gen = this batch's generation.
struct Groups { unsigned long long* head; uint32_t* next; unsigned long long gen; };

void launch_merge_indexed(jg_ctx* ctx, uint32_t eb, void* AP, void* AN, const void* BP, const void* BN, const uint32_t* keys,
                          uint64_t n_rows, uint32_t R, const Groups* g = nullptr) {
    if (g && R >= 32 && ((uint64_t)R * eb) % 16 == 0) {
        JG_REQUIRE(n_rows < kNil, JG_EINVAL, "merge: %llu rows exceed one grouped launch", (unsigned long long)n_rows);
        const unsigned gk = jg::grid_for(ctx, n_rows, kBlock, 16);
        hipLaunchKernelGGL(k_group_link, dim3(gk), dim3(kBlock), 0, ctx->stream, keys, n_rows, g->head, g->next, g->gen);
        constexpr int U = 4;  // rows in flight per wave (U = 8 measured slower, tools/tune_grouped.hip)
        const unsigned grid = jg::grid_for(ctx, (n_rows + U - 1) / U * 64, kBlock, 16);
        jg::dispatch_eb(eb, [&](auto EB) {
            using T = typename Elem<EB()>::T;
            hipLaunchKernelGGL((k_merge_grouped<EB(), U>), dim3(grid), dim3(kBlock), 0, ctx->stream, (T*)AP, (T*)AN, (const T*)BP, (const T*)BN,
                               keys, g->head, g->next, n_rows, R, g->gen);
        });
        JG_HIP(hipGetLastError());
        return;
    }
    if (R >= 32) {
        const unsigned grid = jg::grid_for(ctx, n_rows * 64, kBlock, 16);
        jg::dispatch_eb(eb, [&](auto EB) {
            using T = typename Elem<EB()>::T;
            hipLaunchKernelGGL(k_merge_indexed_rows<EB()>, dim3(grid), dim3(kBlock), 0, ctx->stream, (T*)AP, (T*)AN, (const T*)BP, (const T*)BN,
                               keys, n_rows, R);
        });
        JG_HIP(hipGetLastError());
        return;
    }
    const unsigned grid = jg::grid_for(ctx, n_rows * R, kBlock, 16);
    jg::dispatch_eb(eb, [&](auto EB) {
        using T = typename Elem<EB()>::T;
        hipLaunchKernelGGL(k_merge_indexed<EB()>, dim3(grid), dim3(kBlock), 0, ctx->stream, (T*)AP, (T*)AN, (const T*)BP, (const T*)BN, keys,
                           n_rows, R);
    });
    JG_HIP(hipGetLastError());
}

// The store's group state for a batch of n_rows (allocated on first use; each grouped merge takes the next
// generation, and the heads are cleared once every 2^32 - 1 batches).  nullptr when rows are too narrow
// for the vector path.
const Groups* groups_of(jg_pnc* p, uint64_t n_rows, Groups& g) {
    if (p->R < 32 || ((uint64_t)p->R * p->eb) % 16 != 0) return nullptr;
    if (!p->head.p || p->head_gen == 0xFFFFFFFFull) {
        const bool first = !p->head.p;
        if (first) p->head.alloc(p->n_keys * 8);
        JG_HIP(hipMemsetAsync(p->head.p, 0, p->n_keys * 8, p->ctx->stream));
        p->head_gen = 0;
        // JANUS_TEST_HEAD_GEN: a new store's first generation (tests run batches across the wrap)
        const char* e = first ? std::getenv("JANUS_TEST_HEAD_GEN") : nullptr;
        // clamped below 2^32 - 1: the increment below then gives 1 .. 2^32 - 1, never 0 or 2^32 (a generation
        // whose low 32 bits read 0 would make every head look old)
        if (e) p->head_gen = std::min<unsigned long long>(std::strtoull(e, nullptr, 10), 0xFFFFFFFEull);
    }
    ++p->head_gen;
    if (p->next.bytes < n_rows * 4) {
        JG_HIP(hipStreamSynchronize(p->ctx->stream));  // an earlier launch may still read the old links
        p->next.alloc(n_rows * 4 + n_rows);
    }
    g = Groups{p->head.as<unsigned long long>(), p->next.as<uint32_t>(), p->head_gen};
    return &g;
}

void launch_rows_copy(jg_ctx* ctx, uint32_t eb, void* dst, const void* src, const uint32_t* keys, uint64_t n_rows, uint32_t R,
                      int scatter) {
    const unsigned grid = jg::grid_for(ctx, n_rows * R, kBlock, 16);
    jg::dispatch_eb(eb, [&](auto EB) {
        using T = typename Elem<EB()>::T;
        hipLaunchKernelGGL(k_rows_copy<EB()>, dim3(grid), dim3(kBlock), 0, ctx->stream, (T*)dst, (const T*)src, keys, n_rows, R, scatter);
    });
    JG_HIP(hipGetLastError());
}

template <class T>
void launch_restride_t(jg_ctx* ctx, void* dst, const void* src, uint64_t sw, uint64_t dw, uint64_t src_rows, uint64_t dst_rows) {
    const uint64_t n_units = dst_rows * dw;
    const unsigned grid = (unsigned)std::min<uint64_t>(std::max<uint64_t>((n_units + kBlock - 1) / kBlock, 1), kRestrideBlocks);
    const uint64_t step = (uint64_t)grid * kBlock;
    hipLaunchKernelGGL(k_restride<T>, dim3(grid), dim3(kBlock), 0, ctx->stream, (T*)dst, (const T*)src, (uint32_t)sw, (uint32_t)dw,
                       1.0f / (float)dw, src_rows, n_units, step / dw, (uint32_t)(step % dw));
    JG_HIP(hipGetLastError());
}

// [src_rows x sr] cells of `cell` bytes into [dst_rows x dr] (dr > sr), new cells zero: the vector path where both
// row sizes are whole 16-B vectors (always so for the replica table's Guids), else cell by cell.
void launch_restride(jg_ctx* ctx, uint32_t cell, void* dst, const void* src, uint32_t sr, uint32_t dr, uint64_t src_rows, uint64_t dst_rows) {
    const uint64_t sb = (uint64_t)sr * cell, db = (uint64_t)dr * cell;
    if (sb % 16 == 0 && db % 16 == 0) launch_restride_t<uint4>(ctx, dst, src, sb / 16, db / 16, src_rows, dst_rows);
    else if (cell == 8) launch_restride_t<long long>(ctx, dst, src, sr, dr, src_rows, dst_rows);
    else launch_restride_t<int>(ctx, dst, src, sr, dr, src_rows, dst_rows);
}

// The same rows under more keys (the stride stays): a device copy and the tail zeroed.
void grow_rows(jg_ctx* ctx, void* dst, const void* src, size_t old_bytes, size_t new_bytes) {
    if (old_bytes) JG_HIP(hipMemcpyAsync(dst, src, old_bytes, hipMemcpyDeviceToDevice, ctx->stream));
    if (new_bytes > old_bytes) JG_HIP(hipMemsetAsync((char*)dst + old_bytes, 0, new_bytes - old_bytes, ctx->stream));
}

void swap_buf(jg::DevBuf& a, jg::DevBuf& b) {
    std::swap(a.p, b.p);
    std::swap(a.bytes, b.bytes);
    std::swap(a.own, b.own);
}

// ---- the narrow form of a received batch (jg_rows in jg_internal.hpp, pnc_filter.hpp) ---------------
// An int64 identity batch whose every cell fits is held as 4-byte codes in the lower half of P_ / N_.  It is decided
// where the batch is born: jg_rows_upload narrows each landed chunk under the next chunk's copy, jg_synth_pnc_rows
// writes the codes directly.  rows_wide gives every reader but the dense merge the int64 arrays back.

constexpr size_t kNarrowFlagAt = 128;  // the upload's "a cell does not fit" word in ctx->flags (zero between calls)
// Cells per staged chunk of an upload: at most a quarter of an array (two chunks fit the free upper half), capped at
// 128 MB: every chunk costs the link a launch's worth of host time, and only the last chunk's narrowing (about 50 us
// at the cap) is not hidden under a copy.
constexpr uint64_t kNarrowChunkCap = 16777216;

// codes[i] = narrow(cells[i]) for n cells of a landed chunk; *flag raised if a cell does not fit (every writer
// stores the same value).
__global__ __launch_bounds__(kBlock) void k_rows_narrow(const long long* __restrict__ cells, int* __restrict__ codes, uint64_t n,
                                                        unsigned* __restrict__ flag) {
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const long long b = __builtin_nontemporal_load(cells + i);
        bad |= !jg::filt::fits(b);
        codes[i] = jg::filt::narrow(b);
    }
    if (bad) *flag = 1u;
}

// The same in place over the first n <= kBlock cells of `buf`, one workgroup: every cell is read before any code is
// written (a batch too small to stage in its own upper half).
__global__ __launch_bounds__(kBlock) void k_rows_narrow_small(void* buf, uint32_t n, unsigned* flag) {
    const bool in = threadIdx.x < n;
    const long long b = in ? static_cast<const long long*>(buf)[threadIdx.x] : 0;
    __syncthreads();
    if (in) {
        if (!jg::filt::fits(b)) *flag = 1u;
        static_cast<int*>(buf)[threadIdx.x] = jg::filt::narrow(b);
    }
}

// cells[i] = widen(codes[i]) for i in [lo, hi), both views of one buffer.  The caller keeps 8 lo >= 4 hi: the bytes
// written ([8 lo, 8 hi)) lie behind the bytes read ([4 lo, 4 hi)).
__global__ __launch_bounds__(kBlock) void k_rows_widen(void* buf, uint64_t lo, uint64_t hi) {
    const int* codes = static_cast<const int*>(buf);
    long long* cells = static_cast<long long*>(buf);
    for (uint64_t i = lo + (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < hi; i += (uint64_t)gridDim.x * kBlock)
        cells[i] = jg::filt::widen(codes[i]);
}

// The first n <= kBlock cells, one workgroup: every code is read before any cell is written.
__global__ __launch_bounds__(kBlock) void k_rows_widen_small(void* buf, uint32_t n) {
    const bool in = threadIdx.x < n;
    const int c = in ? static_cast<const int*>(buf)[threadIdx.x] : 0;
    __syncthreads();
    if (in) static_cast<long long*>(buf)[threadIdx.x] = jg::filt::widen(c);
}

// One array widened in place, back to front by halves: the pass over cells [ceil(hi / 2), hi) writes only bytes no
// code of a later pass lies in; a batch of n cells takes log2(n / kBlock) launches (this path is correct, not fast).
void widen_in_place(jg_ctx* ctx, void* buf, uint64_t n_cells) {
    uint64_t hi = n_cells;
    while (hi > (uint64_t)kBlock) {
        const uint64_t lo = (hi + 1) / 2;
        hipLaunchKernelGGL(k_rows_widen, dim3(jg::grid_for(ctx, hi - lo, kBlock, 16)), dim3(kBlock), 0, ctx->stream, buf, lo, hi);
        hi = lo;
    }
    hipLaunchKernelGGL(k_rows_widen_small, dim3(1), dim3(kBlock), 0, ctx->stream, buf, (uint32_t)hi);
    JG_HIP(hipGetLastError());
}

// One host array of n int64 cells into `buf` (8 n bytes) as codes.  Chunk k is copied into staging slot k & 1 of the
// upper half and narrowed into the lower half on one and the same stream, and the chunks alternate between ctx->stream
// and ctx->copy (`turn` runs on across P and N): a chunk's narrowing runs under the next chunk's copy, a slot's next
// copy is ordered behind the kernel that reads it by its stream alone, and between two copies the host issues nothing
// but one launch (a copy from pageable memory holds the host, so every call between two of them idles the link).
void upload_narrow_array(jg_ctx* ctx, unsigned& turn, void* buf, const void* host, uint64_t n) {
    auto* flag = reinterpret_cast<unsigned*>(ctx->flags.as<char>() + kNarrowFlagAt);
    const uint64_t stage_at = jg::round_up(n * 4, 16);                      // behind the codes, vector-aligned
    const uint64_t room = n * 8 > stage_at ? n * 8 - stage_at : 0;          // n = 1: the aligned end lies past the buffer
    const uint64_t chunk = std::min<uint64_t>(room / 16, kNarrowChunkCap);  // two slots of `chunk` cells
    if (chunk == 0) {  // n <= 3: no room to stage
        JG_HIP(hipMemcpyAsync(buf, host, n * 8, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_rows_narrow_small, dim3(1), dim3(kBlock), 0, ctx->stream, buf, (uint32_t)n, flag);
        JG_HIP(hipGetLastError());
        return;
    }
    char* const stage = static_cast<char*>(buf) + stage_at;
    uint64_t k = 0;
    for (uint64_t c0 = 0; c0 < n; c0 += chunk, ++k, ++turn) {
        const uint64_t len = std::min(chunk, n - c0);
        hipStream_t st = (turn & 1) ? ctx->copy : ctx->stream;
        long long* const dst = reinterpret_cast<long long*>(stage + (k & 1) * chunk * 8);
        JG_HIP(hipMemcpyAsync(dst, static_cast<const char*>(host) + c0 * 8, len * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_rows_narrow, dim3(jg::grid_for(ctx, len, kBlock, 8)), dim3(kBlock), 0, st, dst, static_cast<int*>(buf) + c0, len, flag);
    }
    JG_HIP(hipGetLastError());
}

// jg_rows_upload of an int64 identity batch with narrowing on.  true: every cell fitted and the batch holds its codes;
// false: a cell did not fit (the buffers hold partial codes: the caller uploads wide).  Both streams have drained.
bool upload_narrow(jg_rows* r, const void* P, const void* N) {
    jg_ctx* ctx = r->ctx;
    const uint64_t n = r->n_rows * r->R;
    JG_HIP(hipStreamSynchronize(ctx->stream));  // an asynchronous merge may still read the buffers ctx->copy is about to write
    unsigned turn = 0;
    upload_narrow_array(ctx, turn, r->P_.p, P, n);
    upload_narrow_array(ctx, turn, r->N_.p, N, n);
    JG_HIP(hipStreamSynchronize(ctx->copy));
    jg::pin_get(ctx, 0, ctx->flags.as<char>() + kNarrowFlagAt, sizeof(unsigned));
    jg::pin_sync(ctx);
    if (*static_cast<const unsigned*>(jg::pin_at(ctx, 0)) == 0) return true;
    JG_HIP(hipMemsetAsync(ctx->flags.as<char>() + kNarrowFlagAt, 0, sizeof(unsigned), ctx->stream));
    return false;
}

}  // namespace

jg::WideRows jg::rows_wide(const jg_rows* r) {
    if (r->narrow) {
        const uint64_t n = r->n_rows * r->R;
        widen_in_place(r->ctx, r->P_.p, n);
        widen_in_place(r->ctx, r->N_.p, n);
        r->narrow = false;
    }
    return WideRows{r->P_.p, r->N_.p};
}

void jg::pnc_merge_indexed(jg_pnc* p, const void* BP, const void* BN, const uint32_t* d_keys, uint64_t n_rows) {
    Groups g;
    launch_merge_indexed(p->ctx, p->eb, p->rw_P(), p->rw_N(), BP, BN, d_keys, n_rows, p->R, groups_of(p, n_rows, g));
}

// The store grown in place to [n_keys x n_replicas] (never shrunk).  Every new buffer is allocated before anything
// is copied and the store's own fields change only after both streams have drained, so a failure at any point
// leaves the store as it was (the new buffers are freed on the way out).  Takes no heed of an open wave: the
// public entry point refuses those, the automatic widening runs inside one (pnc_auto_widen).
void jg::pnc_grow(jg_pnc* p, uint64_t n_keys, uint32_t n_replicas) {
    const uint64_t ok = p->n_keys, nk = std::max(n_keys, ok);
    const uint32_t orr = p->R, nr = std::max(n_replicas, orr), eb = p->eb;
    if (nk == ok && nr == orr) return;
    JG_REQUIRE(nk <= 0xFFFFFFFFull, JG_EINVAL, "jg_pnc_reserve: key_idx is 32-bit (%llu keys)", (unsigned long long)nk);
    JG_REQUIRE(nr < 0x40000000u, JG_EINVAL, "jg_pnc_reserve: at most 2^30-1 replica columns");  // k_restride's index arithmetic
    JG_REQUIRE(!p->cols.p || nr <= jg::kMaxTableReplicas, JG_EINVAL, "jg_pnc_reserve: the replica table holds at most %u replicas per key (%u asked)",
               jg::kMaxTableReplicas, nr);
    JG_REQUIRE(nk * nr <= (1ull << 44), JG_ENOMEM, "jg_pnc_reserve: %llu x %u cells exceed any device", (unsigned long long)nk, nr);
    jg_ctx* ctx = p->ctx;
    jg::ensure_device(ctx);
    const bool table = p->cols.p != nullptr;
    static const bool trace = std::getenv("JANUS_TRACE_RESERVE") != nullptr;  // the call's phases to stderr
    const double t0 = jg::now_us();
    jg::DevBuf nP, nN, nC, nNc;  // all of them first: an allocation failure leaves the store untouched
    nP.alloc((size_t)nk * nr * eb);
    nN.alloc((size_t)nk * nr * eb);
    if (table) {
        nC.alloc((size_t)nk * nr * 16);
        nNc.alloc((size_t)nk * 4);
    }
    if (nr == orr) {
        grow_rows(ctx, nP.p, p->ro_P(), (size_t)ok * orr * eb, nP.bytes);
        grow_rows(ctx, nN.p, p->ro_N(), (size_t)ok * orr * eb, nN.bytes);
        if (table) grow_rows(ctx, nC.p, p->cols.p, (size_t)ok * orr * 16, nC.bytes);
    } else {
        launch_restride(ctx, eb, nP.p, p->ro_P(), orr, nr, ok, nk);
        launch_restride(ctx, eb, nN.p, p->ro_N(), orr, nr, ok, nk);
        if (table) launch_restride(ctx, 16, nC.p, p->cols.p, orr, nr, ok, nk);  // new slots all-zero (json_wave.hpp row_cache)
    }
    if (table) grow_rows(ctx, nNc.p, p->ncols.p, (size_t)ok * 4, nNc.bytes);
    const double t1 = jg::now_us();
    // the old buffers go: everything queued on them first (an async merge_batch on `stream`, the upload stream)
    JG_HIP(hipStreamSynchronize(ctx->stream));
    JG_HIP(hipStreamSynchronize(ctx->copy));
    const double t2 = jg::now_us();
    swap_buf(p->P_, nP);
    swap_buf(p->N_, nN);
    if (table) swap_buf(p->cols, nC), swap_buf(p->ncols, nNc);
    if (nk != ok) p->head.release();  // the grouped merge's heads follow n_keys: first use recreates them (groups_of)
    drop_shadow(p);  // the dense merge's shadow follows the shape (both streams have drained: nothing reads it)
    p->n_keys = nk;
    p->R = nr;
    if (trace) {
        nP.release(), nN.release(), nC.release(), nNc.release();  // the old buffers (freed here or on the way out)
        std::fprintf(stderr, "reserve %llu x %u -> %llu x %u: allocate + queue %.3f ms, copies %.3f ms, free %.3f ms\n", (unsigned long long)ok, orr,
                     (unsigned long long)nk, nr, (t1 - t0) * 1e-3, (t2 - t1) * 1e-3, (jg::now_us() - t2) * 1e-3);
    }
}

// One step of the opt-in widening after a call failed for row capacity (its roll-back has run): R doubles, up to
// the caller's bound and the replica table's.  false = at the bound (or no room on the device): the call's own
// failure stands.
bool jg::pnc_auto_widen(jg_pnc* p) {
    uint64_t cap = p->max_R;
    if (p->cols.p) cap = std::min<uint64_t>(cap, jg::kMaxTableReplicas);
    const uint64_t nr = std::min<uint64_t>(2ull * p->R, cap);
    if (nr <= p->R) return false;
    try {
        pnc_grow(p, p->n_keys, (uint32_t)nr);
    } catch (const jg::Error&) {
        return false;
    }
    return true;
}

extern "C" {

int jg_pnc_create(jg_ctx* ctx, uint64_t n_keys, uint32_t n_replicas, uint32_t elem_bytes, jg_pnc** out) {
    return jg::guard([&] {
        auto lk_ = jg::lock(ctx);  // calls on one context are serialised (shared scratch, stream)
        JG_REQUIRE(ctx && out, JG_EINVAL, "jg_pnc_create: NULL argument");
        JG_REQUIRE(elem_bytes == 4 || elem_bytes == 8, JG_EINVAL, "jg_pnc_create: elem_bytes must be 4 or 8");
        JG_REQUIRE(n_replicas > 0 && n_keys > 0, JG_EINVAL, "jg_pnc_create: empty shape");
        JG_REQUIRE(n_keys <= 0xFFFFFFFFull, JG_EINVAL, "jg_pnc_create: key_idx is 32-bit");
        jg::ensure_device(ctx);
        auto* p = new jg_pnc();
        p->ctx = ctx; p->n_keys = n_keys; p->R = n_replicas; p->eb = elem_bytes;
        try {
            const size_t bytes = (size_t)n_keys * n_replicas * elem_bytes;
            p->P_.alloc(bytes);
            p->N_.alloc(bytes);
            JG_HIP(hipMemsetAsync(p->rw_P(), 0, bytes, ctx->stream));  // PNCounter(): every replica absent = 0
            JG_HIP(hipMemsetAsync(p->rw_N(), 0, bytes, ctx->stream));
            JG_HIP(hipStreamSynchronize(ctx->stream));
        } catch (...) {
            delete p;
            throw;
        }
        *out = p;
    });
}

int jg_pnc_destroy(jg_pnc* p) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        jg::require_writable(p, "jg_pnc_destroy");
        if (!p) return;
        jg::ensure_device(p->ctx);
        JG_HIP(hipStreamSynchronize(p->ctx->stream));
        delete p;
    });
}

int jg_pnc_shape(jg_pnc* p, uint64_t* n_keys, uint32_t* n_replicas, uint32_t* elem_bytes) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        check_store(p, "jg_pnc_shape");
        if (n_keys) *n_keys = p->n_keys;
        if (n_replicas) *n_replicas = p->R;
        if (elem_bytes) *elem_bytes = p->eb;
    });
}

int jg_pnc_reserve(jg_pnc* p, uint64_t n_keys, uint32_t n_replicas) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        jg::require_writable(p, "jg_pnc_reserve");
        check_store(p, "jg_pnc_reserve");
        JG_REQUIRE(!p->wopen, JG_EINVAL, "jg_pnc_reserve: a wave (jg_pnc_wave_begin) is open on this store");
        jg::pnc_grow(p, n_keys, n_replicas);
    });
}

int jg_pnc_set_max_replicas(jg_pnc* p, uint32_t max_replicas) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        check_store(p, "jg_pnc_set_max_replicas");
        p->max_R = max_replicas;
    });
}

int jg_pnc_set_dense_filter(jg_pnc* p, int on) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        check_store(p, "jg_pnc_set_dense_filter");
        p->filt_on = on != 0;
        if (!p->filt_on) {
            jg::ensure_device(p->ctx);
            JG_HIP(hipStreamSynchronize(p->ctx->stream));  // an asynchronous merge may still read the shadow
            drop_shadow(p);
        }
    });
}

int jg_pnc_dense_filter_state(jg_pnc* p, int* state) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        check_store(p, "jg_pnc_dense_filter_state");
        JG_REQUIRE(state, JG_EINVAL, "jg_pnc_dense_filter_state: NULL output");
        *state = p->filt_on ? p->filt : 0;
    });
}

int jg_pnc_write_rows(jg_pnc* p, const uint32_t* key_idx, uint64_t n_rows, const void* P, const void* N) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        jg::require_writable(p, "jg_pnc_write_rows");
        check_store(p, "jg_pnc_write_rows");
        JG_REQUIRE(P && N, JG_EINVAL, "jg_pnc_write_rows: NULL rows");
        if (n_rows == 0) return;
        jg_ctx* ctx = p->ctx;
        jg::ensure_device(ctx);
        const size_t bytes = (size_t)n_rows * p->R * p->eb;
        if (!key_idx) {
            JG_REQUIRE(n_rows <= p->n_keys, JG_EINVAL, "jg_pnc_write_rows: %llu rows > n_keys", (unsigned long long)n_rows);
            JG_HIP(hipMemcpyAsync(p->rw_P(), P, bytes, hipMemcpyHostToDevice, ctx->stream));
            JG_HIP(hipMemcpyAsync(p->rw_N(), N, bytes, hipMemcpyHostToDevice, ctx->stream));
        } else {
            const uint32_t* dk = upload_keys(ctx, key_idx, n_rows, p->n_keys, "jg_pnc_write_rows");
            void* st = jg::scratch(ctx, ctx->scratch2, 2 * bytes);
            JG_HIP(hipMemcpyAsync(st, P, bytes, hipMemcpyHostToDevice, ctx->stream));
            JG_HIP(hipMemcpyAsync((char*)st + bytes, N, bytes, hipMemcpyHostToDevice, ctx->stream));
            launch_rows_copy(ctx, p->eb, p->rw_P(), st, dk, n_rows, p->R, 1);
            launch_rows_copy(ctx, p->eb, p->rw_N(), (char*)st + bytes, dk, n_rows, p->R, 1);
        }
        JG_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int jg_pnc_read_rows(jg_pnc* p, const uint32_t* key_idx, uint64_t n_rows, void* P, void* N) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        check_store(p, "jg_pnc_read_rows");
        JG_REQUIRE(P && N, JG_EINVAL, "jg_pnc_read_rows: NULL rows");
        if (n_rows == 0) return;
        jg_ctx* ctx = p->ctx;
        jg::ensure_device(ctx);
        const size_t bytes = (size_t)n_rows * p->R * p->eb;
        if (!key_idx) {
            JG_REQUIRE(n_rows <= p->n_keys, JG_EINVAL, "jg_pnc_read_rows: %llu rows > n_keys", (unsigned long long)n_rows);
            JG_HIP(hipMemcpyAsync(P, p->ro_P(), bytes, hipMemcpyDeviceToHost, ctx->stream));
            JG_HIP(hipMemcpyAsync(N, p->ro_N(), bytes, hipMemcpyDeviceToHost, ctx->stream));
        } else {
            const uint32_t* dk = upload_keys(ctx, key_idx, n_rows, p->n_keys, "jg_pnc_read_rows");
            void* st = jg::scratch(ctx, ctx->scratch2, 2 * bytes);
            launch_rows_copy(ctx, p->eb, st, p->ro_P(), dk, n_rows, p->R, 0);
            launch_rows_copy(ctx, p->eb, (char*)st + bytes, p->ro_N(), dk, n_rows, p->R, 0);
            JG_HIP(hipMemcpyAsync(P, st, bytes, hipMemcpyDeviceToHost, ctx->stream));
            JG_HIP(hipMemcpyAsync(N, (char*)st + bytes, bytes, hipMemcpyDeviceToHost, ctx->stream));
        }
        JG_HIP(hipStreamSynchronize(ctx->stream));
    });
}

}  // extern "C"

namespace jg {
void pnc_values_device(jg_pnc* p, const uint32_t* d_keys, uint64_t n, long long* d_out, uint8_t* d_ovf, const uint32_t* d_at,
                       const unsigned long long* d_count, uint8_t of_code) {
    jg_ctx* ctx = p->ctx;
    const unsigned grid = jg::grid_for(ctx, n * 64, kBlock, 16);
    dispatch_eb(p->eb, [&](auto EB) {
        using T = typename Elem<EB()>::T;
        hipLaunchKernelGGL(k_values<EB()>, dim3(grid), dim3(kBlock), 0, ctx->stream, (const T*)p->ro_P(), (const T*)p->ro_N(), p->R, d_keys, n, d_out,
                           d_ovf, d_at, d_count, of_code);
    });
    JG_HIP(hipGetLastError());
}
}  // namespace jg

extern "C" {

int jg_pnc_merge_rows(jg_pnc* p, const uint32_t* key_idx, uint64_t n_rows, const void* P, const void* N) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        jg::require_writable(p, "jg_pnc_merge_rows");
        check_store(p, "jg_pnc_merge_rows");
        JG_REQUIRE(P && N, JG_EINVAL, "jg_pnc_merge_rows: NULL rows");
        if (n_rows == 0) return;
        jg_ctx* ctx = p->ctx;
        jg::ensure_device(ctx);
        const size_t bytes = (size_t)n_rows * p->R * p->eb;
        const uint32_t* dk = nullptr;
        if (key_idx) dk = upload_keys(ctx, key_idx, n_rows, p->n_keys, "jg_pnc_merge_rows");
        else JG_REQUIRE(n_rows <= p->n_keys, JG_EINVAL, "jg_pnc_merge_rows: %llu rows > n_keys", (unsigned long long)n_rows);
        void* st = jg::scratch(ctx, ctx->scratch2, 2 * bytes);
        JG_HIP(hipMemcpyAsync(st, P, bytes, hipMemcpyHostToDevice, ctx->stream));
        JG_HIP(hipMemcpyAsync((char*)st + bytes, N, bytes, hipMemcpyHostToDevice, ctx->stream));
        Groups g;
        if (dk) launch_merge_indexed(ctx, p->eb, p->rw_P(), p->rw_N(), st, (char*)st + bytes, dk, n_rows, p->R, groups_of(p, n_rows, g));
        else merge_dense_store(p, st, (char*)st + bytes, n_rows);
        JG_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int jg_pnc_apply_ops(jg_pnc* p, uint64_t n_ops, const uint32_t* key, const uint32_t* col, const int64_t* delta, const uint8_t* is_n) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        jg::require_writable(p, "jg_pnc_apply_ops");
        check_store(p, "jg_pnc_apply_ops");
        if (n_ops == 0) return;
        JG_REQUIRE(key && col && delta && is_n, JG_EINVAL, "jg_pnc_apply_ops: NULL argument");
        for (uint64_t i = 0; i < n_ops; ++i)
            JG_REQUIRE(key[i] < p->n_keys && col[i] < p->R, JG_EINVAL, "jg_pnc_apply_ops: op %llu addresses (%u,%u) outside the store",
                       (unsigned long long)i, key[i], col[i]);
        jg_ctx* ctx = p->ctx;
        jg::ensure_device(ctx);
        uint32_t *dkey, *dcol;
        long long* ddel;
        uint8_t* dn;
        jg::Layout L;
        L.add(dkey, n_ops, 16), L.add(dcol, n_ops, 4), L.add(ddel, n_ops, 16), L.add(dn, n_ops, 1);
        L.bind(jg::scratch(ctx, ctx->scratch2, L.bytes() + 64));
        JG_HIP(hipMemcpyAsync(dkey, key, n_ops * 4, hipMemcpyHostToDevice, ctx->stream));
        JG_HIP(hipMemcpyAsync(dcol, col, n_ops * 4, hipMemcpyHostToDevice, ctx->stream));
        JG_HIP(hipMemcpyAsync(ddel, delta, n_ops * 8, hipMemcpyHostToDevice, ctx->stream));
        JG_HIP(hipMemcpyAsync(dn, is_n, n_ops, hipMemcpyHostToDevice, ctx->stream));
        const unsigned grid = jg::grid_for(ctx, n_ops, kBlock, 16);
        jg::dispatch_eb(p->eb, [&](auto EB) {
            using T = typename Elem<EB()>::T;
            hipLaunchKernelGGL(k_apply_ops<EB()>, dim3(grid), dim3(kBlock), 0, ctx->stream, (T*)p->rw_P(), (T*)p->rw_N(), dkey, dcol, ddel, dn, n_ops,
                               p->R);
        });
        JG_HIP(hipGetLastError());
        JG_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int jg_pnc_values(jg_pnc* p, const uint32_t* key_idx, uint64_t n, int64_t* out, uint8_t* overflow) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        check_store(p, "jg_pnc_values");
        JG_REQUIRE(out && overflow, JG_EINVAL, "jg_pnc_values: NULL output");
        if (n == 0) return;
        jg_ctx* ctx = p->ctx;
        jg::ensure_device(ctx);
        const uint32_t* dk = nullptr;
        if (key_idx) dk = upload_keys(ctx, key_idx, n, p->n_keys, "jg_pnc_values");
        else JG_REQUIRE(n <= p->n_keys, JG_EINVAL, "jg_pnc_values: %llu keys > n_keys", (unsigned long long)n);
        char* st = static_cast<char*>(jg::scratch(ctx, ctx->scratch2, n * 9 + 64));
        long long* dout = (long long*)st;
        uint8_t* dovf = (uint8_t*)(st + n * 8);
        jg::pnc_values_device(p, dk, n, dout, dovf, nullptr, nullptr, 1);
        JG_HIP(hipMemcpyAsync(out, dout, n * 8, hipMemcpyDeviceToHost, ctx->stream));
        JG_HIP(hipMemcpyAsync(overflow, dovf, n, hipMemcpyDeviceToHost, ctx->stream));
        JG_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int jg_rows_create(jg_ctx* ctx, uint64_t n_rows, uint32_t n_replicas, uint32_t elem_bytes, jg_rows** out) {
    return jg::guard([&] {
        auto lk_ = jg::lock(ctx);  // calls on one context are serialised (shared scratch, stream)
        JG_REQUIRE(ctx && out, JG_EINVAL, "jg_rows_create: NULL argument");
        JG_REQUIRE(elem_bytes == 4 || elem_bytes == 8, JG_EINVAL, "jg_rows_create: elem_bytes must be 4 or 8");
        JG_REQUIRE(n_rows > 0 && n_replicas > 0, JG_EINVAL, "jg_rows_create: empty shape");
        jg::ensure_device(ctx);
        auto* r = new jg_rows();
        r->ctx = ctx; r->n_rows = n_rows; r->R = n_replicas; r->eb = elem_bytes;
        try {
            const size_t bytes = (size_t)n_rows * n_replicas * elem_bytes;
            r->P_.alloc(bytes);
            r->N_.alloc(bytes);
        } catch (...) {
            delete r;
            throw;
        }
        *out = r;
    });
}

int jg_rows_destroy(jg_rows* r) {
    return jg::guard([&] {
        auto lk_ = jg::lock(r);  // calls on one context are serialised (shared scratch, stream)
        if (!r) return;
        jg::ensure_device(r->ctx);
        JG_HIP(hipStreamSynchronize(r->ctx->stream));
        delete r;
    });
}

int jg_rows_upload(jg_rows* r, const uint32_t* key_idx, const void* P, const void* N) {
    return jg::guard([&] {
        auto lk_ = jg::lock(r);  // calls on one context are serialised (shared scratch, stream)
        JG_REQUIRE(r && P && N, JG_EINVAL, "jg_rows_upload: NULL argument");
        jg_ctx* ctx = r->ctx;
        jg::ensure_device(ctx);
        const size_t bytes = (size_t)r->n_rows * r->R * r->eb;
        r->narrow = false;
        // an int64 identity batch is narrowed chunk by chunk as it lands; one that holds a cell that does not fit is
        // copied again, wide (rare: correct, not fast), as every keyed and every int32 batch is in the first place
        if (!key_idx && r->eb == 8 && r->narrow_on) r->narrow = upload_narrow(r, P, N);
        if (!r->narrow) {
            JG_HIP(hipMemcpyAsync(r->P_.p, P, bytes, hipMemcpyHostToDevice, ctx->stream));
            JG_HIP(hipMemcpyAsync(r->N_.p, N, bytes, hipMemcpyHostToDevice, ctx->stream));
        }
        if (key_idx) {
            uint32_t mx = 0;
            for (uint64_t i = 0; i < r->n_rows; ++i) mx = key_idx[i] > mx ? key_idx[i] : mx;
            r->max_key = mx;
            if (r->keys.bytes < r->n_rows * 4) r->keys.alloc(r->n_rows * 4);
            JG_HIP(hipMemcpyAsync(r->keys.p, key_idx, r->n_rows * 4, hipMemcpyHostToDevice, ctx->stream));
            r->has_keys = true;
        } else {
            r->has_keys = false;
        }
        JG_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int jg_pnc_merge_batch(jg_pnc* p, const jg_rows* r, int async) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        jg::require_writable(p, "jg_pnc_merge_batch");
        check_store(p, "jg_pnc_merge_batch");
        JG_REQUIRE(r, JG_EINVAL, "jg_pnc_merge_batch: rows is NULL");
        JG_REQUIRE(r->ctx == p->ctx, JG_EINVAL, "jg_pnc_merge_batch: rows and store belong to different contexts");
        JG_REQUIRE(r->R == p->R && r->eb == p->eb, JG_ETYPE, "jg_pnc_merge_batch: row shape (%u x %uB) != store (%u x %uB)", r->R, r->eb,
                   p->R, p->eb);
        jg_ctx* ctx = p->ctx;
        jg::ensure_device(ctx);
        if (r->has_keys) {
            JG_REQUIRE(r->max_key < p->n_keys, JG_EINVAL, "jg_pnc_merge_batch: batch addresses key %u >= n_keys %llu", r->max_key,
                       (unsigned long long)p->n_keys);
            Groups g;
            const jg::WideRows w = jg::rows_wide(r);  // a keyed batch is wide already
            launch_merge_indexed(ctx, p->eb, p->rw_P(), p->rw_N(), w.P, w.N, r->keys.as<uint32_t>(), r->n_rows, p->R, groups_of(p, r->n_rows, g));
        } else {
            JG_REQUIRE(r->n_rows <= p->n_keys, JG_EINVAL, "jg_pnc_merge_batch: identity batch of %llu rows > n_keys",
                       (unsigned long long)r->n_rows);
            merge_dense_store(p, r->P_.p, r->N_.p, r->n_rows, r->narrow);  // the one reader of either form in place
        }
        if (!async) JG_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int jg_rows_set_narrow(jg_rows* r, int on) {
    return jg::guard([&] {
        auto lk_ = jg::lock(r);  // calls on one context are serialised (shared scratch, stream)
        JG_REQUIRE(r, JG_EINVAL, "jg_rows_set_narrow: rows is NULL");
        r->narrow_on = on != 0;
        if (!r->narrow_on && r->narrow) {
            jg::ensure_device(r->ctx);
            jg::rows_wide(r);
            JG_HIP(hipStreamSynchronize(r->ctx->stream));
        }
    });
}

int jg_rows_form(jg_rows* r, int* form) {
    return jg::guard([&] {
        auto lk_ = jg::lock(r);  // calls on one context are serialised (shared scratch, stream)
        JG_REQUIRE(r && form, JG_EINVAL, "jg_rows_form: NULL argument");
        *form = r->narrow ? 1 : 0;
    });
}

}  // extern "C"
