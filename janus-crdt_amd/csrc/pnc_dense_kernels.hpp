// pnc_dense_kernels.hpp — every kernel of the dense PN-Counter merge (A = max(A, B) over identity rows) and of the
// received batch's two forms, with their shape constants: the plain merge, the merge through the 32-bit shadow
// (pnc_filter.hpp: the build launch that creates it, the filtered kernel that merges by it, the clamp pass over rows a
// batch did not cover) and the passes that narrow and widen a batch.  csrc/pnc_dense.hip launches them; tools/tune_pnc.hip
// compiles the same text beside its variants; no other file includes it (some kernels here are no templates).
//
// Invariant of a valid shadow: S[c] == clamp32(A[c]) for every cell c of the store.  Every kernel here keeps it for
// the cells it touches; any other writer of A drops the shadow on the host (jg_pnc::rw_P / rw_N).
#pragma once

#include <type_traits>

#include "pnc_filter.hpp"
#include "pnc_vec.hpp"

namespace jg {
namespace filt {

typedef long long v2ll __attribute__((ext_vector_type(2)));
typedef int v2i __attribute__((ext_vector_type(2)));
typedef int v4i __attribute__((ext_vector_type(4)));

// A lane's CPL consecutive cells (CPL = 2 | 4): int64 cells as CPL / 2 16-B vectors, their shadows as one 8-B or
// 16-B vector.
template <int CPL> __device__ __forceinline__ void ld_cells(const long long* X, uint64_t unit, long long (&x)[CPL]) {
#pragma unroll
    for (int k = 0; k < CPL / 2; ++k) {
        const v2ll v = nt_ld(reinterpret_cast<const v2ll*>(X) + unit * (CPL / 2) + k);
        x[2 * k] = v.x, x[2 * k + 1] = v.y;
    }
}
template <int CPL> __device__ __forceinline__ void st_cells(long long* X, uint64_t unit, const long long (&x)[CPL]) {
#pragma unroll
    for (int k = 0; k < CPL / 2; ++k) nt_st(reinterpret_cast<v2ll*>(X) + unit * (CPL / 2) + k, v2ll{x[2 * k], x[2 * k + 1]});
}
template <int CPL> __device__ __forceinline__ void ld_shadow(const int* S, uint64_t unit, int (&s)[CPL]) {
    if constexpr (CPL == 2) {
        const v2i v = nt_ld(reinterpret_cast<const v2i*>(S) + unit);
        s[0] = v.x, s[1] = v.y;
    } else {
        const v4i v = nt_ld(reinterpret_cast<const v4i*>(S) + unit);
        s[0] = v.x, s[1] = v.y, s[2] = v.z, s[3] = v.w;
    }
}
template <int CPL> __device__ __forceinline__ void st_shadow(int* S, uint64_t unit, const int (&s)[CPL]) {
    if constexpr (CPL == 2) nt_st(reinterpret_cast<v2i*>(S) + unit, v2i{s[0], s[1]});
    else nt_st(reinterpret_cast<v4i*>(S) + unit, v4i{s[0], s[1], s[2], s[3]});
}

// A lane's CPL consecutive int64 cells of the received batch in its form (jg_rows): BT = long long, the cells
// themselves; BT = int, the narrow form's 4-byte codes (pnc_filter.hpp `narrow`), one 8-B or 16-B vector widened in
// registers.  batch_cell: one cell of a store of T cells; a batch of cells as wide as T holds them as they are (the
// wide form, and every int32 batch).
template <int CPL, class BT> __device__ __forceinline__ void ld_batch(const BT* B, uint64_t unit, long long (&b)[CPL]) {
    if constexpr (sizeof(BT) == 8) {
        ld_cells<CPL>(B, unit, b);
    } else {
        int c[CPL];
        ld_shadow<CPL>(B, unit, c);
#pragma unroll
        for (int k = 0; k < CPL; ++k) b[k] = widen(c[k]);
    }
}
template <class T = long long, class BT> __device__ __forceinline__ T batch_cell(const BT* B, uint64_t at) {
    if constexpr (sizeof(BT) == sizeof(T)) return B[at];
    else return (T)widen(B[at]);
}

// ---- the plain merge ---------------------------------------------------------------------------------------------
// Dense merge: nv 16-byte vectors per array plus `tail` trailing cells (< 16 B) done by block 0.  The grid is two
// halves of `half` workgroups (layout.hpp halves_of): the first merges P (A.P, B.P), the second N (A.N, B.N), so in
// dispatch order the chip streams two arrays at a time, then the other two, instead of four at once.  A workgroup takes
// kDenseVecs vectors per lane, kDenseBlock apart (a wave-instruction reads 1 KB contiguous, an aligned group of
// kElideLanes lanes is one 128-B line), every load issued before the first use.  Measured on MI355X in the regime the
// kernel now mostly runs in — four read streams, nothing stored — and behind batches that raise one column per key or
// every cell (tools/tune_pnc.hip `steady`, profiles/r08/tune_pnc_steady*.txt), against the four-streams-per-workgroup
// shape it had since round 1 and against 2 / 4 vectors per lane, workgroups of 512 / 1024, bounded grids (grid-stride
// and block-chunk walks), P then N inside a workgroup, default-policy loads and LDS-DMA loads: see DESIGN.md §4 for
// what each measured.  P and N are elided separately (each half writes only its own array); the bounds test is a
// predicate, not a branch around the ballot, so every lane of a wave that loaded data votes (lanes past nv vote
// unchanged).
constexpr int kDenseVecs = 1;     // 16-B vectors of each array per lane
constexpr int kDenseBlock = 256;  // lanes per workgroup: kDenseVecs x kDenseBlock vectors per workgroup

// BV: the batch beside A's 16-B vectors.  uint4: the batch's own cells (the wide form, and every int32 batch).  uint2
// (int64 stores only): two 4-byte codes of a narrow batch (jg_rows), widened in registers.
template <int EB, class BV>
__device__ __forceinline__ void merge_dense_body(uint4* __restrict__ AP, uint4* __restrict__ AN, const BV* __restrict__ BP,
                                                 const BV* __restrict__ BN, uint64_t nv, uint32_t tail, uint32_t half) {
    using T = std::conditional_t<EB == 8, long long, int>;
    using BT = std::conditional_t<sizeof(BV) == 16, T, int>;  // the batch's cell type
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
        if (in[u]) {
            a[u] = nt_ld(A + i);
            if constexpr (sizeof(BV) == 16) {
                b[u] = nt_ld(B + i);
            } else {
                long long c[2];
                ld_batch<2>(reinterpret_cast<const int*>(B), i, c);
                b[u] = __builtin_bit_cast(uint4, I64x2{c[0], c[1]});
            }
        }
    }
    const uint32_t lane = threadIdx.x & 63;
#pragma unroll
    for (int u = 0; u < kDenseVecs; ++u) {
        const uint4 m = vmax<EB>(a[u], b[u]);
        const unsigned long long c = __ballot(in[u] && differs(m, a[u]));
        if (in[u] && group_any<kElideLanes>(c, lane)) nt_st(A + base + u * kDenseBlock, m);
    }
    if (blockIdx.x == 0 && threadIdx.x < tail) {
        T* ap = reinterpret_cast<T*>(AP + nv) + threadIdx.x;
        T* an = reinterpret_cast<T*>(AN + nv) + threadIdx.x;
        const T bp = batch_cell<T>(reinterpret_cast<const BT*>(BP + nv), threadIdx.x);
        const T bn = batch_cell<T>(reinterpret_cast<const BT*>(BN + nv), threadIdx.x);
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

// ---- the merge by the 32-bit shadow (int64 stores) --------------------------------------------------
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
// The filtered kernel's shape for a narrow batch (4-byte codes of B beside the 4-byte shadow: two equal read streams),
// chosen like the wide batch's in tools/tune_pnc.hip `narrow`.
constexpr int kNarrowCells = 2;
constexpr int kNarrowVecs = 2;
constexpr int kNarrowBlock = 256;

// One trailing cell (the cells past the last whole unit, one lane each), by the shadow: scalar and exact.
__device__ __forceinline__ void merge_tail_cell(long long* a, int* s, long long b) {
    const int sv = *s;
    if (!may_change(sv, b)) return;
    const Merged r = merge_cell(known(sv) ? (long long)sv : *a, b);
    if (r.changed) *a = r.m, *s = r.s;
}

// The filtered merge over n_units units of CPL cells per array plus `tail` trailing cells (< CPL).  The grid is two
// halves of `half` workgroups as k_merge_dense's: P's, then N's.  A lane reads the shadows and B of VECS units,
// BLOCK apart, every load issued before the first use, and A only for a 128-B line that holds an escape cell while
// a cell of the line may change (rare: the escape path is exact, not fast).  A line of A is written whole or not at
// all; the shadow's 64 B of the line are written with it.  BT: the batch's cell type (ld_batch); everything after the
// load is the same code for both forms.
template <int CPL, int VECS, int BLOCK, class BT = long long>
__global__ __launch_bounds__(BLOCK) void k_merge_filtered(long long* __restrict__ AP, long long* __restrict__ AN, int* __restrict__ SP,
                                                          int* __restrict__ SN, const BT* __restrict__ BP,
                                                          const BT* __restrict__ BN, uint64_t n_units, uint32_t tail, uint32_t half) {
    constexpr uint32_t G = 16 / CPL;
    const bool isN = blockIdx.x >= half;
    long long* const A = isN ? AN : AP;
    int* const S = isN ? SN : SP;
    const BT* const B = isN ? BN : BP;
    const uint32_t blk = blockIdx.x - (isN ? half : 0);
    const uint64_t base = (uint64_t)blk * (VECS * BLOCK) + threadIdx.x;
    int s[VECS][CPL];
    long long b[VECS][CPL];
    bool in[VECS];
#pragma unroll
    for (int u = 0; u < VECS; ++u) {
        const uint64_t i = base + u * BLOCK;
        in[u] = i < n_units;
#pragma unroll
        for (int k = 0; k < CPL; ++k) s[u][k] = 0, b[u][k] = INT64_MIN;  // a lane past the end: nothing may change
        if (in[u]) ld_shadow<CPL>(S, i, s[u]), ld_batch<CPL>(B, i, b[u]);
    }
    const uint32_t lane = threadIdx.x & 63;
#pragma unroll
    for (int u = 0; u < VECS; ++u) {
        const uint64_t i = base + u * BLOCK;
        bool may = false, esc = false;
#pragma unroll
        for (int k = 0; k < CPL; ++k) may |= may_change(s[u][k], b[u][k]), esc |= !known(s[u][k]);
        const unsigned long long mm = __ballot(may), me = __ballot(esc);
        long long a[CPL];
#pragma unroll
        for (int k = 0; k < CPL; ++k) a[k] = s[u][k];
        if (in[u] && group_any<G>(mm, lane) && group_any<G>(me, lane)) ld_cells<CPL>(A, i, a);  // the whole line reads A
        long long m[CPL];
        int ns[CPL];
        bool ch = false;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            const Merged r = merge_cell(a[k], b[u][k]);
            m[k] = r.m, ns[k] = r.s, ch |= r.changed;
        }
        const unsigned long long c = __ballot(ch);
        if (in[u] && group_any<G>(c, lane)) st_cells<CPL>(A, i, m), st_shadow<CPL>(S, i, ns);
    }
    if (blk == 0 && threadIdx.x < tail) {
        const uint64_t at = n_units * CPL + threadIdx.x;
        merge_tail_cell(A + at, S + at, batch_cell(B, at));
    }
}

// The build launch: k_merge_dense's int64 merge (A and B read, the raised 128-B lines of A written back) plus the
// shadow of every cell of the batch, written unconditionally.  Two cells per lane, two halves.  BT as above.
template <int BLOCK, class BT = long long>
__global__ __launch_bounds__(BLOCK) void k_merge_build(long long* __restrict__ AP, long long* __restrict__ AN, int* __restrict__ SP,
                                                       int* __restrict__ SN, const BT* __restrict__ BP, const BT* __restrict__ BN,
                                                       uint64_t n_units, uint32_t tail, uint32_t half) {
    const bool isN = blockIdx.x >= half;
    long long* const A = isN ? AN : AP;
    int* const S = isN ? SN : SP;
    const BT* const B = isN ? BN : BP;
    const uint32_t blk = blockIdx.x - (isN ? half : 0);
    const uint64_t i = (uint64_t)blk * BLOCK + threadIdx.x;
    const bool in = i < n_units;
    long long a[2] = {0, 0}, b[2] = {INT64_MIN, INT64_MIN};
    if (in) ld_cells<2>(A, i, a), ld_batch<2>(B, i, b);
    const Merged r0 = merge_cell(a[0], b[0]), r1 = merge_cell(a[1], b[1]);
    const unsigned long long c = __ballot(r0.changed || r1.changed);
    if (in) {
        const long long m[2] = {r0.m, r1.m};
        const int ns[2] = {r0.s, r1.s};
        if (group_any<kElideLanes>(c, threadIdx.x & 63)) st_cells<2>(A, i, m);
        st_shadow<2>(S, i, ns);
    }
    if (blk == 0 && threadIdx.x < tail) {
        const uint64_t at = n_units * 2 + threadIdx.x;
        const Merged r = merge_cell(A[at], batch_cell(B, at));
        if (r.changed) A[at] = r.m;
        S[at] = r.s;
    }
}

// S[c] = clamp32(A[c]) for cells [from, to): the rows of the store behind a batch shorter than the store.
__global__ __launch_bounds__(256) void k_shadow_clamp(const long long* __restrict__ A, int* __restrict__ S, uint64_t from, uint64_t to) {
    for (uint64_t c = from + (uint64_t)blockIdx.x * 256 + threadIdx.x; c < to; c += (uint64_t)gridDim.x * 256) S[c] = clamp32(A[c]);
}

// ---- the batch's two forms (jg_rows; pnc_filter.hpp fits / narrow / widen) ----------------------------------------
constexpr int kRowsBlock = 256;  // lanes per workgroup of the passes below

// codes[i] = narrow(cells[i]) for n cells of a landed chunk; *flag raised if a cell does not fit (every writer
// stores the same value).
__global__ __launch_bounds__(kRowsBlock) void k_rows_narrow(const long long* __restrict__ cells, int* __restrict__ codes, uint64_t n,
                                                                   unsigned* __restrict__ flag) {
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * kRowsBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kRowsBlock) {
        const long long b = nt_ld(cells + i);
        bad |= !fits(b);
        codes[i] = narrow(b);
    }
    if (bad) *flag = 1u;
}

// The same in place over the first n <= kRowsBlock cells of `buf`, one workgroup: every cell is read before any code
// is written (a batch too small to stage in its own upper half).
__global__ __launch_bounds__(kRowsBlock) void k_rows_narrow_small(void* buf, uint32_t n, unsigned* flag) {
    const bool in = threadIdx.x < n;
    const long long b = in ? static_cast<const long long*>(buf)[threadIdx.x] : 0;
    __syncthreads();
    if (in) {
        if (!fits(b)) *flag = 1u;
        static_cast<int*>(buf)[threadIdx.x] = narrow(b);
    }
}

// cells[i] = widen(codes[i]) for i in [lo, hi), both views of one buffer.  The caller keeps 8 lo >= 4 hi: the bytes
// written ([8 lo, 8 hi)) lie behind the bytes read ([4 lo, 4 hi)).
__global__ __launch_bounds__(kRowsBlock) void k_rows_widen(void* buf, uint64_t lo, uint64_t hi) {
    const int* codes = static_cast<const int*>(buf);
    long long* cells = static_cast<long long*>(buf);
    for (uint64_t i = lo + (uint64_t)blockIdx.x * kRowsBlock + threadIdx.x; i < hi; i += (uint64_t)gridDim.x * kRowsBlock)
        cells[i] = widen(codes[i]);
}

// The first n <= kRowsBlock cells, one workgroup: every code is read before any cell is written.
__global__ __launch_bounds__(kRowsBlock) void k_rows_widen_small(void* buf, uint32_t n) {
    const bool in = threadIdx.x < n;
    const int c = in ? static_cast<const int*>(buf)[threadIdx.x] : 0;
    __syncthreads();
    if (in) static_cast<long long*>(buf)[threadIdx.x] = widen(c);
}

}  // namespace filt
}  // namespace jg
