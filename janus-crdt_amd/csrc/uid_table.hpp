// uid_table.hpp — a node's uid table on the device (uid -> PN-Counter row | OR-Set set id) and its probe, shared by
// the wave path (node.hip, which owns the table: host copy authoritative, dirty slots uploaded by sync_table), the
// reads and writes by key name (query.hip, update.hip) and creation on the device (adopt.hip, whose kernels insert into
// the device copy; node.hip stores the slots they claimed into the host copy).
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

// node.hip, for adopt.hip: the node's uid table as kernels insert into it.  node_insert_begin refuses an open
// streamed wave of the node and a wave holding either store, grows the host table for `n_more` more uids, uploads
// every pending registration and hands out the device copy.  The kernels then claim free slots (uid_claim) for uids the
// table lacks; node_insert_commit stores those (slot, entry) pairs into the host copy without probing again — slot[i]
// kNoSlot: item i inserted nothing — and moves the node's counts, allocation marks and shard flag as jg_node_register
// would have.  Nothing else may touch the node between the two.
struct NodeInsert {
    jg_ctx* ctx;
    jg_pnc* pnc;
    jg_orset* orset;
    UidSlot* tab;
    uint64_t mask;
    uint32_t next_row, next_set;  // one past the largest row / set id registered by any path, 0 with none
};
NodeInsert node_insert_begin(jg_node* nd, uint64_t n_more, const char* fn);
void node_insert_commit(jg_node* nd, uint64_t n, const jg_guid* uid, const uint32_t* slot, const uint32_t* val);
void node_next_idx(const jg_node* nd, uint32_t* next_row, uint32_t* next_set);

// A free slot of the table for the uid (lo, hi), which the table lacks, claimed against the other lanes of the launch
// through the slot's pad0 word: an entry's uid may have a zero half, so neither half can be the CAS target.  A slot is
// free while its uid is zero and its pad0 is; the claimant writes the entry afterwards (a lane that reads a half-written
// uid sees an occupied slot, which is what it is).  pad0 stays set on the device copy; nothing else reads it, and a
// re-upload of the slot from the host copy writes 0 beside a uid that is not zero.
__device__ __forceinline__ uint32_t uid_claim(UidSlot* tab, uint64_t mask, unsigned long long lo, unsigned long long hi) {
    for (uint64_t q = uid_hash(lo, hi) & mask;; q = (q + 1) & mask) {
        const UidSlot e = tab[q];
        if ((e.lo | e.hi) == 0 && e.pad0 == 0 && atomicCAS(&tab[q].pad0, 0u, 1u) == 0u) return (uint32_t)q;
    }
}

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
