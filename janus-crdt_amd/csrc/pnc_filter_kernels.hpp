// pnc_filter_kernels.hpp — the dense int64 PN-Counter merge through the 32-bit shadow (pnc_filter.hpp): the build
// launch that creates the shadow, the filtered kernel that merges by it, and the clamp pass over rows a batch did
// not cover.  Templates over the shape so that csrc/pnc.hip and tools/tune_pnc.hip (`filter` mode) compile the same
// text.  gfx950, wave64, plain HIP.
//
// Invariant of a valid shadow: S[c] == clamp32(A[c]) for every cell c of the store.  Every kernel here keeps it for
// the cells it touches; any other writer of A drops the shadow on the host (jg_pnc::rw_P / rw_N).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pnc_filter.hpp"

namespace jg {
namespace filt {

typedef long long v2ll __attribute__((ext_vector_type(2)));
typedef int v2i __attribute__((ext_vector_type(2)));
typedef int v4i __attribute__((ext_vector_type(4)));

// A lane's CPL consecutive cells (CPL = 2 | 4): int64 cells as CPL / 2 16-B vectors, their shadows as one 8-B or
// 16-B vector; non-temporal (every byte is touched once per launch).
template <int CPL> __device__ __forceinline__ void ld_cells(const long long* X, uint64_t unit, long long (&x)[CPL]) {
#pragma unroll
    for (int k = 0; k < CPL / 2; ++k) {
        const v2ll v = __builtin_nontemporal_load(reinterpret_cast<const v2ll*>(X) + unit * (CPL / 2) + k);
        x[2 * k] = v.x, x[2 * k + 1] = v.y;
    }
}
template <int CPL> __device__ __forceinline__ void st_cells(long long* X, uint64_t unit, const long long (&x)[CPL]) {
#pragma unroll
    for (int k = 0; k < CPL / 2; ++k) __builtin_nontemporal_store(v2ll{x[2 * k], x[2 * k + 1]}, reinterpret_cast<v2ll*>(X) + unit * (CPL / 2) + k);
}
template <int CPL> __device__ __forceinline__ void ld_shadow(const int* S, uint64_t unit, int (&s)[CPL]) {
    if constexpr (CPL == 2) {
        const v2i v = __builtin_nontemporal_load(reinterpret_cast<const v2i*>(S) + unit);
        s[0] = v.x, s[1] = v.y;
    } else {
        const v4i v = __builtin_nontemporal_load(reinterpret_cast<const v4i*>(S) + unit);
        s[0] = v.x, s[1] = v.y, s[2] = v.z, s[3] = v.w;
    }
}
template <int CPL> __device__ __forceinline__ void st_shadow(int* S, uint64_t unit, const int (&s)[CPL]) {
    if constexpr (CPL == 2) __builtin_nontemporal_store(v2i{s[0], s[1]}, reinterpret_cast<v2i*>(S) + unit);
    else __builtin_nontemporal_store(v4i{s[0], s[1], s[2], s[3]}, reinterpret_cast<v4i*>(S) + unit);
}

// A lane's CPL consecutive cells of the received batch in its form (jg_rows): BT = long long, the cells themselves;
// BT = int, the narrow form's 4-byte codes (pnc_filter.hpp `narrow`), one 8-B or 16-B vector widened in registers.
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
template <class BT> __device__ __forceinline__ long long batch_cell(const BT* B, uint64_t at) {
    if constexpr (sizeof(BT) == 8) return B[at];
    else return widen(B[at]);
}

// Any lane of this lane's aligned group of G lanes set in the wave's ballot `mask` (G lanes x CPL cells = one 128-B
// line of A: the unit a store is elided by, as k_merge_dense's kElideLanes).
template <uint32_t G> __device__ __forceinline__ bool group_any(unsigned long long mask, uint32_t lane) {
    return ((mask >> (lane & (64 - G))) & ((1u << G) - 1)) != 0;
}

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
        if (group_any<8>(c, threadIdx.x & 63)) st_cells<2>(A, i, m);
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

}  // namespace filt
}  // namespace jg
