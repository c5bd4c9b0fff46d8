// pnc_vec.hpp — the 16-B vector helpers the PN-Counter merge kernels share (pnc_dense_kernels.hpp; k_merge_grouped and
// k_restride in pnc.hip): non-temporal loads and stores, the cell-wise maximum, and store elision's lane-group predicate.
#pragma once

#include <hip/hip_runtime.h>

namespace jg::filt {

typedef unsigned int v4u __attribute__((ext_vector_type(4)));

// Non-temporal loads and stores (every byte is touched once per launch): any scalar or ext-vector type, and uint4.
template <class T> __device__ __forceinline__ T nt_ld(const T* p) { return __builtin_nontemporal_load(p); }
template <> __device__ __forceinline__ uint4 nt_ld<uint4>(const uint4* p) {
    return __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const v4u*>(p)));
}
template <class T> __device__ __forceinline__ void nt_st(T* p, T v) { __builtin_nontemporal_store(v, p); }
template <> __device__ __forceinline__ void nt_st<uint4>(uint4* p, uint4 v) {
    __builtin_nontemporal_store(__builtin_bit_cast(v4u, v), reinterpret_cast<v4u*>(p));
}

// Store elision (merge kernels): max is idempotent and most merges are no-ops for most cells (a replica advances its
// own column only, every message is a full state, anti-entropy re-delivers merged states), so a vector of A is stored
// only if its aligned group of G lanes holds a lane whose maximum differs from what it loaded: G lanes x 16 B = one
// 128-B line (kElideLanes lanes of a 16-B vector each, 16 / CPL lanes of CPL int64 cells) where the lanes' vectors are
// consecutive and the group's first is line-aligned (the dense kernels always; k_merge_grouped where the row is a
// multiple of 128 B), so a line is written whole or not at all.  Granularity measured against per-lane (16 B) and
// per-wave (1 KB) elision over 0 - 100 % changed cells (tools/tune_pnc.hip, profiles/r07/tune_pnc_elide.txt).
// Correctness rests on neither grouping nor alignment: a lane that stores writes the maximum, a lane that skips held an
// unchanged value.  `mask` is the wave's ballot of changed lanes (inactive lanes read as unchanged); group_any: any
// lane of this lane's aligned group of G lanes is set in it.
constexpr uint32_t kElideLanes = 8;
template <uint32_t G> __device__ __forceinline__ bool group_any(unsigned long long mask, uint32_t lane) {
    if constexpr (G == 64) return mask != 0;
    else return ((mask >> (lane & (64 - G))) & ((1u << G) - 1)) != 0;
}

struct I64x2 { long long x, y; };
struct I32x4 { int x, y, z, w; };

// The cell-wise maximum of two 16-B vectors of EB-byte cells.
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

// True where the two vectors differ in any bit.
__device__ __forceinline__ bool differs(uint4 a, uint4 b) { return ((a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w)) != 0; }

}  // namespace jg::filt
