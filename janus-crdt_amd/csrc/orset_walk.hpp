// orset_walk.hpp — the index arithmetic of the OR-Set record walk on the device (orset_walk.hip).
// HIP-free: host/test_orset_walk.cpp compiles it with g++ alone (and under the sanitizers) and holds it to a
// sequential walk; the kernels call the same functions.
//
// The walk in prefix-sum form.  Ops are ordered by (set, elem, Clear epoch, op index); a SEGMENT is one (set, elem,
// epoch).  For a segment with stored tag sets A0 / R0 (empty unless the epoch is 0 and the batch Removes or reads the
// key): nA0 = |A0|, nR0 = |R0|, m0 = |R0 \ A0|, u0 = |A0 \ R0|.  An Add ISSUES when its tag is not in A0 and is the
// first of its tag in the segment, FILLS when it issues and the tag is in R0, and is a U-ADD when it issues and does
// not fill.  At position p of the segment:
//     nA = nA0 + issues before p                m = m0 - fills before p
//     u  = u-adds since the last Remove before p (+ u0 if there is none)
//     nR = nR0 + (u0 + u-adds before that Remove, if there is one)
// A Remove issues u tombstones (u0's tags by (ord, tag) if it is the first, then the u-adds in op order).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define JGW_HD __host__ __device__ __forceinline__
#else
#define JGW_HD inline
#endif

namespace jgw {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kNullElem = 0xFFFFFFFFu;  // JG_NULL_ELEM

// The last p in [0, n) with off[p] <= j, for off non-decreasing with off[0] <= j (n >= 1): the owner of item j among
// segments whose exclusive offsets are off[] — a segment of length 0 never owns an item.
JGW_HD uint64_t last_le(const unsigned long long* off, uint64_t n, unsigned long long j) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (off[mid] <= j) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Marks for the inclusive max-scan that finds the last Remove before a position: a Remove at p marks 2p + 1, a
// segment's first position 2p, anything else 0 (p < 2^31).
JGW_HD uint32_t mark(uint32_t p, bool seg_head, bool is_remove) { return is_remove ? 2u * p + 1u : seg_head ? 2u * p : 0u; }

// The last Remove strictly before p inside p's segment (which starts at seg), from the scanned marks; kNone: none.
JGW_HD uint32_t prev_remove(const uint32_t* scanned, uint32_t p, uint32_t seg) {
    if (p == seg) return kNone;
    const uint32_t m = scanned[p - 1];
    return (m & 1u) && (m >> 1) >= seg ? (m >> 1) : kNone;
}

// Reversed marks for the scan that finds the next Remove: position p goes to slot n - 1 - p and marks slot + 1 if it is
// a Remove; the inclusive max-scan at p's slot then names the first Remove at or after p.
JGW_HD uint32_t rev_slot(uint32_t n, uint32_t p) { return n - 1u - p; }
JGW_HD uint32_t rev_mark(uint32_t n, uint32_t p, bool is_remove) { return is_remove ? rev_slot(n, p) + 1u : 0u; }
JGW_HD uint32_t next_remove(const uint32_t* scanned, uint32_t n, uint32_t p) {
    const uint32_t v = scanned[rev_slot(n, p)];
    return v ? n - v : kNone;
}

struct Base { uint64_t nA0, nR0, m0, u0; };
struct State { uint64_t nA, nR, m, u; };

// is / fl / ua: issues, fills and u-adds of the segment before the position; has_rm: a Remove precedes it in the
// segment, with ua_rm u-adds of the segment before that Remove.
JGW_HD State state_at(const Base& b, uint64_t is, uint64_t fl, uint64_t ua, bool has_rm, uint64_t ua_rm) {
    State s;
    s.nA = b.nA0 + is;
    s.m = b.m0 - fl;
    s.u = has_rm ? ua - ua_rm : b.u0 + ua;
    s.nR = has_rm ? b.nR0 + b.u0 + ua_rm : b.nR0;
    return s;
}

// ORSet.Contains at that state (ORSet.cs:204-237): the null element is present iff its tag sets differ; any other
// element iff it has an add tag and (no tombstone or the sets differ).
JGW_HD bool present(uint32_t elem, const State& s) {
    const bool differ = s.m > 0 || s.u > 0;
    return elem == kNullElem ? differ : s.nA > 0 && (s.nR == 0 || differ);
}

// The local index, inside its Remove's block of tombstone ords, of a u-add with ua u-adds of the segment before it:
// the first Remove of a segment puts the u0 stored tags first.
JGW_HD uint64_t uadd_slot(const Base& b, uint64_t ua, bool has_rm, uint64_t ua_rm) { return has_rm ? ua - ua_rm : b.u0 + ua; }

}  // namespace jgw
