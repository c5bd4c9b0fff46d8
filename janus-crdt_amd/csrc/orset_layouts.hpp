// orset_layouts.hpp — the OR-Set wave path's carved blocks, each described once: the description gives the block's
// size (allocation, memset) and, bound to a base, its pointers.  No HIP type: host/test_layout.cpp holds the offsets
// and sizes to the formulas written out there, with g++ alone.
#pragma once

#include <cstring>

#include "layout.hpp"

namespace jg {

// The slots a wave table's inserts claimed are appended to kLists sub-lists (orset_tables.hpp list_append).
constexpr uint32_t kLists = 16;

// The bucket counts the tables' claimants take (Claims, orset_tables.hpp; the bucket commit's Buckets start with
// the same four): arrays of cap + 1 entries — new strings per set, records per set for the two sides, then the new
// strings' bytes.  One block (jg_orset_wire::cbc), zeroed whole per wave.  Returns the block's bytes; with a base,
// c.scnt, c.rcnt[0], c.rcnt[1] and c.sbytes point into it.
template <class C> size_t carve_claims(uint64_t cap, void* base, C& c) {
    Layout L;
    L.add(c.scnt, cap + 1), L.add(c.rcnt[0], cap + 1), L.add(c.rcnt[1], cap + 1), L.add(c.sbytes, cap + 1);
    if (base) L.bind(base);
    return L.bytes();
}

// The bucket commit's places and bucket orders (Buckets, orset_commit.hpp) for every entry the two tables' lists can
// hold: sub-lists of cap / 8 entries (a table is at most half full) and one spare.  One block (jg_orset_wire::cb).
// Returns the block's bytes; with a base, b.spos ... b.ritem[1] point into it.
template <class B> size_t carve_items(uint64_t st_cap, uint64_t rt_cap, void* base, B& b) {
    const uint64_t s = (st_cap / 8) * kLists + 1, r = (rt_cap / 8) * kLists + 1;
    Layout L;
    L.add(b.spos, s), L.add(b.sset, s), L.add(b.sitem, s);
    L.add(b.rpos, r), L.add(b.rset, r), L.add(b.ritem[0], r), L.add(b.ritem[1], r);
    if (base) L.bind(base);
    return L.bytes();
}

// Page-locked staging of n names with nb pool bytes: set [n] u32 | id [n] u32 | len [n] u32 | pad to 16 |
// pool offset [n] u64 | pool bytes [nb].
struct NamesStaging {
    uint64_t n;
    size_t set, id, len, pool_off, pool, bytes;
    NamesStaging(uint64_t n_, uint64_t nb)
        : n(n_), set(0), id(n_ * 4), len(n_ * 8), pool_off(round_up(n_ * 12, 16)), pool(pool_off + n_ * 8), bytes(pool + nb) {}
    // A filled block h into the caller's arrays: sets, ids, exclusive byte offsets and the names' bytes back to back
    // (each name's pool offset is absolute; the staged pool bytes start at pool_base).  Returns the bytes written.
    uint64_t copy_out(const uint8_t* h, uint64_t pool_base, uint32_t* oset, uint32_t* oid, uint64_t* ooff, uint8_t* obytes) const {
        const auto* hlen = reinterpret_cast<const uint32_t*>(h + len);  // h is 16-byte aligned: so are len and pool_off
        const auto* hat = reinterpret_cast<const uint64_t*>(h + pool_off);
        std::memcpy(oset, h + set, n * 4);
        std::memcpy(oid, h + id, n * 4);
        ooff[0] = 0;
        for (uint64_t i = 0; i < n; ++i) {
            ooff[i + 1] = ooff[i] + hlen[i];
            if (hlen[i]) std::memcpy(obytes + ooff[i], h + pool + (hat[i] - pool_base), hlen[i]);
        }
        return ooff[n];
    }
};

}  // namespace jg
