// orset_view.hpp — the read side of an OR-Set record stream in the CHUNKED layout (orset_union.hpp describes it): tags,
// the view a kernel takes by value, rank -> slot, a key's run in rank space, and the Clear drop bitmap.  No kernel is
// defined here, so every unit that only reads streams (orset_walk.hip) includes this file alone.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace jgk {

constexpr int kQShift = 9;  // LUT granularity: one entry per 512 ranks

struct Tag { unsigned long long lo, hi; };

__device__ __forceinline__ Tag ld_tag(const uint4* p) { return __builtin_bit_cast(Tag, *p); }
typedef unsigned int nt_v4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ Tag ld_tag_nt(const uint4* p) {
    return __builtin_bit_cast(Tag, __builtin_nontemporal_load(reinterpret_cast<const nt_v4u*>(p)));
}
// Streams' records read through global-address-space pointers: a pointer picked per lane between two
// streams is otherwise generic (a FLAT load, which also counts on lgkmcnt).
template <class T>
using gptr = const __attribute__((address_space(1))) T*;
template <class T>
__device__ __forceinline__ gptr<T> as_global(const T* p) { return (gptr<T>)p; }
__device__ __forceinline__ Tag ld_tag_nt(gptr<uint4> p) {
    return __builtin_bit_cast(Tag, __builtin_nontemporal_load((gptr<nt_v4u>)p));
}
__device__ __forceinline__ void st_tag_nt(uint4* p, uint4 v) {
    __builtin_nontemporal_store(__builtin_bit_cast(nt_v4u, v), reinterpret_cast<nt_v4u*>(p));
}
__device__ __forceinline__ uint4 to_u4(Tag t) { return __builtin_bit_cast(uint4, t); }

// Branch-free lexicographic compare on (key, tag.lo, tag.hi), unsigned.
__device__ __forceinline__ bool rec_lt(unsigned long long ka, Tag ta, unsigned long long kb, Tag tb) {
    return (ka < kb) | ((ka == kb) & ((ta.lo < tb.lo) | ((ta.lo == tb.lo) & (ta.hi < tb.hi))));
}
__device__ __forceinline__ bool rec_eq(unsigned long long ka, Tag ta, unsigned long long kb, Tag tb) {
    return (ka == kb) & (ta.lo == tb.lo) & (ta.hi == tb.hi);
}

// Read view of one chunked stream (plain pointers: passed by value to kernels).
struct View {
    const unsigned long long* key;
    const uint4* tag;
    const uint32_t* ord;  // arrival ordinals (jg_tagrec.ord); only the union reads them
    const uint64_t* off;  // [nch + 1]
    const uint32_t* lut;  // [(n >> kQShift) + 2]
    uint64_t n;
    uint32_t nch;
    uint32_t C;
    uint32_t dense;  // 1: off[c] = c*C (slot = rank), set for uploaded and generated streams
};

__device__ __forceinline__ uint32_t chunk_of(const View& v, uint64_t r) {  // r < n: the last chunk with off <= r
    if (v.dense) return (uint32_t)(r / v.C);
    const uint64_t q = r >> kQShift;
    uint32_t lo = v.lut[q], hi = v.lut[q + 1];
    while (lo < hi) {
        const uint32_t m = (lo + hi + 1) >> 1;
        if (v.off[m] <= r) lo = m;
        else hi = m - 1;
    }
    return lo;
}
__device__ __forceinline__ uint64_t slot_of(const View& v, uint64_t r) {
    if (v.dense) return r;
    const uint32_t c = chunk_of(v, r);
    return (uint64_t)c * v.C + (r - v.off[c]);
}

// A key's run in rank space: the key at rank r, the first rank whose key is >= q, the first whose key is > q.
__device__ __forceinline__ unsigned long long key_at(const View& v, uint64_t r) { return v.key[slot_of(v, r)]; }
__device__ __forceinline__ uint64_t lower_key(const View& v, unsigned long long q) {
    uint64_t lo = 0, hi = v.n;
    while (lo < hi) { const uint64_t m = (lo + hi) >> 1; if (key_at(v, m) < q) lo = m + 1; else hi = m; }
    return lo;
}
__device__ __forceinline__ uint64_t upper_key(const View& v, unsigned long long q) {
    uint64_t lo = 0, hi = v.n;
    while (lo < hi) { const uint64_t m = (lo + hi) >> 1; if (key_at(v, m) <= q) lo = m + 1; else hi = m; }
    return lo;
}

// Set-indexed drop bitmap (ORSet.Clear applied inside a batch of ops): A-side records whose set bit
// is 1 are removed from the union; sets past the bitmap's `words` are kept.  nullptr = keep all.
struct Drop {
    const unsigned* bits;
    uint32_t words;
};
__device__ __forceinline__ bool dropped(const Drop& d, unsigned long long key) {
    const unsigned set = (unsigned)(key >> 32);
    return d.bits && (set >> 5) < d.words && ((d.bits[set >> 5] >> (set & 31)) & 1u);
}

}  // namespace jgk
