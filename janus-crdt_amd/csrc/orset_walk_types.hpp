// orset_walk_types.hpp — what the two device forms of the OR-Set record walk share (orset_walk.hip, the multi-launch
// form; orset_walk_small.hip, the one-launch form, §19): the records they sort with their orders, the
// search of a tag in a key's stored run, and the stored state a segment starts from.  HIP only; the index arithmetic
// proper is in orset_walk.hpp and orset_walk_small.hpp, which are HIP-free.
#pragma once

#include "orset_view.hpp"
#include "orset_walk.hpp"

namespace jgw {

// One Add (cls 0) or other op (cls 1) for the tag sort: by (cls, key, epoch, tag, op index).
struct TagRec {
    unsigned long long key, lo, hi;
    uint32_t epoch_cls;  // cls << 31 | epoch
    uint32_t idx;
};
struct TagLess {
    __host__ __device__ bool operator()(const TagRec& a, const TagRec& b) const {
        const uint32_t ca = a.epoch_cls >> 31, cb = b.epoch_cls >> 31;
        if (ca != cb) return ca < cb;
        if (a.key != b.key) return a.key < b.key;
        if (a.epoch_cls != b.epoch_cls) return a.epoch_cls < b.epoch_cls;
        if (a.lo != b.lo) return a.lo < b.lo;
        if (a.hi != b.hi) return a.hi < b.hi;
        return a.idx < b.idx;
    }
};
// One stored add tag of a key the batch Removes or reads: seg = the key's first position in P2, or kNone when the tag has
// a tombstone (not in U0); by (seg, ord, tag).
struct Item {
    uint32_t seg, ord;
    unsigned long long lo, hi;
};
struct ItemLess {
    __host__ __device__ bool operator()(const Item& a, const Item& b) const {
        if (a.seg != b.seg) return a.seg < b.seg;
        if (a.ord != b.ord) return a.ord < b.ord;
        if (a.lo != b.lo) return a.lo < b.lo;
        return a.hi < b.hi;
    }
};
// One tombstone of the batch; by (key, tag).
struct Tomb {
    unsigned long long key, lo, hi;
    uint32_t ord, pad;
};
struct TombLess {
    __host__ __device__ bool operator()(const Tomb& a, const Tomb& b) const {
        if (a.key != b.key) return a.key < b.key;
        if (a.lo != b.lo) return a.lo < b.lo;
        return a.hi < b.hi;
    }
};

// The first rank in [lo, end) of v whose tag is not below t (sorted by tag inside one key's run).
__device__ __forceinline__ uint64_t lower_tag(const jgk::View& v, uint64_t lo, uint64_t end, unsigned long long tlo, unsigned long long thi) {
    uint64_t hi = end;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        const jgk::Tag g = jgk::ld_tag(v.tag + jgk::slot_of(v, mid));
        if (g.lo < tlo || (g.lo == tlo && g.hi < thi)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// Whether tag t is in ranks [lo, end) of v.
__device__ __forceinline__ bool has_tag(const jgk::View& v, uint64_t lo, uint64_t end, unsigned long long tlo, unsigned long long thi) {
    lo = lower_tag(v, lo, end, tlo, thi);
    if (lo >= end) return false;
    const jgk::Tag g = jgk::ld_tag(v.tag + jgk::slot_of(v, lo));
    return g.lo == tlo && g.hi == thi;
}

// What a position's segment starts from: the stored runs in epoch 0 of a key a Remove or a read names, else nothing.
// bnd[4 ks ..]: the rank bounds of the key's stored add run and tombstone run; u0: its stored add tags without a tombstone.
__device__ __forceinline__ Base base_of(uint32_t ks, bool store, const unsigned long long* __restrict__ bnd, uint32_t u0) {
    Base b{0, 0, 0, 0};
    if (store) {
        b.nA0 = bnd[4 * (uint64_t)ks + 1] - bnd[4 * (uint64_t)ks];
        b.nR0 = bnd[4 * (uint64_t)ks + 3] - bnd[4 * (uint64_t)ks + 2];
        b.u0 = u0;
        b.m0 = b.nR0 - (b.nA0 - b.u0);  // |R0| - |A0 ∩ R0|
    }
    return b;
}

}  // namespace jgw
