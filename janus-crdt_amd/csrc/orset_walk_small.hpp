// orset_walk_small.hpp — the index arithmetic of the one-launch OR-Set record walk (orset_walk_small.hip, DESIGN.md
// §19) beyond orset_walk.hpp's.  HIP-free: host/test_orset_walk_small.cpp compiles it with g++ alone (and under the
// sanitizers) and holds it to a sequential restatement; the kernel calls the same functions over LDS arrays.
//
// One workgroup of kThreads threads walks a batch of at most kMaxOps ops, one op per thread in each of the two orders.
// The stored add tags of the keys a Remove or a read names are expanded into kMaxStored items, kItemsPerThread per
// thread in blocked order (thread t owns items kItemsPerThread t ..).  A key's stored run is sorted by tag, so an
// item's index j orders the items of one key by tag: the (seg, ord, tag) order of U0 is the order of the word
// seg << (12 + ord_bits) | ord << 12 | j, which a block radix sort of plain integers gives.  The sorts run over the
// bits in use only: the host passes the widths of the batch's largest set id and element id and of the store's ords.
#pragma once

#include <cstddef>
#include <cstdint>

#include "orset_walk.hpp"

namespace jgs {

constexpr uint32_t kThreads = 1024;   // the workgroup (16 waves)
constexpr uint32_t kMaxOps = 1024;    // kWalkSmallMaxOps: one op per thread
constexpr uint32_t kMaxStored = 4096; // kWalkSmallMaxStored
constexpr uint32_t kItemsPerThread = kMaxStored / kThreads;

// ---- the packed upload: the five input arrays of n ops in one block, widest first so each stays aligned ----
struct Upload {
    size_t lo, hi, set, elem, op, bytes;
};
constexpr Upload upload_layout(uint64_t n) { return Upload{0, (size_t)(8 * n), (size_t)(16 * n), (size_t)(20 * n), (size_t)(24 * n), (size_t)(25 * n)}; }

// ---- the sort word of a stored item ----
// The bits that hold every value below or equal to x (at least 1).
JGW_HD int bits_for(unsigned long long x) {
    int b = 1;
    while (b < 64 && (x >> b) != 0) ++b;
    return b;
}
constexpr int kItemIdxBits = 12, kItemSegBits = 12;
constexpr uint32_t kItemNoSeg = (1u << kItemSegBits) - 1u;  // an item with a tombstone, or a slot past the batch's items: sorts last
static_assert(kMaxStored <= (1u << kItemIdxBits), "an item's index fits its field");
static_assert(kMaxOps < kItemNoSeg, "a position of the batch is below the sentinel");
// ord_bits: the width of the ord field (every ord given is below 1 << ord_bits, ord_bits <= 32)
JGW_HD unsigned long long item_key(uint32_t seg, uint32_t ord, uint32_t j, int ord_bits) {
    return ((unsigned long long)seg << (kItemIdxBits + ord_bits)) | ((unsigned long long)ord << kItemIdxBits) | j;
}
JGW_HD int item_key_bits(int ord_bits) { return kItemIdxBits + ord_bits + kItemSegBits; }
JGW_HD uint32_t item_seg(unsigned long long k, int ord_bits) { return (uint32_t)(k >> (kItemIdxBits + ord_bits)); }
JGW_HD uint32_t item_idx(unsigned long long k) { return (uint32_t)(k & ((1u << kItemIdxBits) - 1u)); }

// ---- the sort word of an op in order 2: (set, elem) in set_bits + elem_bits bits, the key set << 32 | elem back ----
JGW_HD unsigned long long op_key(uint32_t set, uint32_t elem, int elem_bits) { return ((unsigned long long)set << elem_bits) | elem; }
JGW_HD unsigned long long op_key_wide(unsigned long long k, int elem_bits) {
    return ((k >> elem_bits) << 32) | (k & ((1ull << elem_bits) - 1ull));
}

JGW_HD bool tag_lt(unsigned long long alo, unsigned long long ahi, unsigned long long blo, unsigned long long bhi) {
    return alo < blo || (alo == blo && ahi < bhi);
}

// ---- segment-local loops over the (set, elem, epoch, op index) order; lo / hi: the positions' tags ----
// Whether an Add of tag t stands in [b, p): the Add at p is then not the first of its tag in its segment [b, ..).
JGW_HD bool seen_before(const uint8_t* op, const unsigned long long* lo, const unsigned long long* hi, uint32_t b, uint32_t p, unsigned long long tlo,
                        unsigned long long thi) {
    for (uint32_t q = b; q < p; ++q)
        if (op[q] == 1 && lo[q] == tlo && hi[q] == thi) return true;
    return false;
}
// The flagged positions of the segment starting at s (positions q >= s with seg[q] == s, q < n) whose tag is below t: a
// flagged record's rank by tag among its segment's.
JGW_HD uint32_t rank_in_segment(const uint8_t* flag, const uint16_t* seg, const unsigned long long* lo, const unsigned long long* hi, uint32_t n,
                                uint32_t s, unsigned long long tlo, unsigned long long thi) {
    uint32_t r = 0;
    for (uint32_t q = s; q < n && seg[q] == s; ++q)
        if (flag[q] && tag_lt(lo[q], hi[q], tlo, thi)) ++r;
    return r;
}

// ---- three exclusive sums in one scan: issues, fills and u-adds, 16 bits apart (each below kMaxOps + 1) ----
JGW_HD unsigned long long pack3(bool is, bool fl, bool ua) { return (is ? 1ull : 0ull) | (fl ? 1ull << 16 : 0ull) | (ua ? 1ull << 32 : 0ull); }
JGW_HD uint32_t sum_is(unsigned long long v) { return (uint32_t)(v & 0xFFFFu); }
JGW_HD uint32_t sum_fl(unsigned long long v) { return (uint32_t)((v >> 16) & 0xFFFFu); }
JGW_HD uint32_t sum_ua(unsigned long long v) { return (uint32_t)((v >> 32) & 0xFFFFu); }

}  // namespace jgs
