// uid_table.hpp — a node's uid table on the device (uid -> PN-Counter row | OR-Set set id) and its probe, shared by
// the wave path (node.hip, which owns the table: host copy authoritative, dirty slots uploaded by sync_table) and
// the reads by key name (query.hip).
#pragma once

#include <memory>

#include "jg_internal.hpp"

namespace jg {

constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
constexpr uint32_t kOrSetBit = 0x80000000u;  // val = set id | kOrSetBit for an ORSet, the row for a PNCounter

struct UidSlot {
    unsigned long long lo, hi;
    uint32_t val, pad0;
    unsigned long long pad1;
};
static_assert(sizeof(UidSlot) == 32, "one uid slot = half a 64-B line");

struct DevUids { const UidSlot* tab; uint64_t mask; };

// TryGetValue on the uid table: the slot's val, kNoSlot if the uid was never registered (linear probing; the table
// is at most half full, an empty slot is the zero Guid, which is never registered)
__device__ __forceinline__ uint32_t uid_find(const DevUids& u, unsigned long long lo, unsigned long long hi) {
    for (uint64_t q = uid_hash(lo, hi) & u.mask;; q = (q + 1) & u.mask) {
        const UidSlot e = u.tab[q];
        if ((e.lo | e.hi) == 0) return kNoSlot;
        if (e.lo == lo && e.hi == hi) return e.val;
    }
}

// node.hip, for query.hip: the node's stores and its uid table with every registration uploaded (sync_table).
// Refused (JG_EINVAL) while a streamed wave of the node is open and registrations are pending: the open wave
// classifies its remaining chunks against the table it began with.
struct NodeRef {
    jg_ctx* ctx;
    jg_pnc* pnc;
    jg_orset* orset;
    DevUids uids;
    uint32_t max_set;  // the largest set id registered (0 without one)
};
jg_ctx* node_ctx(const jg_node* nd);
NodeRef node_query_ref(jg_node* nd, const char* fn);

// What jg_node_update_keys_ship (update.hip) keeps on the node from one call to the next: the merged image of the last
// call's snapshots, held for jg_node_shipped while `held`, and the regions the rounds' OR-Set states are written to
// (reused, grown as needed).
struct ShipState {
    DevBuf image;
    uint64_t bytes = 0;
    bool held = false;
    std::vector<std::unique_ptr<DevBuf>> region;
};
ShipState& node_ship(jg_node* nd);

}  // namespace jg
