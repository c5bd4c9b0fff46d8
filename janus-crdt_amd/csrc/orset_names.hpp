// orset_names.hpp — the OR-Set element table's layout and probes, and its host owner jg::ElemTable (orset_names.hip),
// used by the wave path (orset_wire.hip), the by-name entry points (orset_names.hip), the encoder (orset_encode.hip)
// and the reads by key name (query.hip).
//
// Element table (per store, first use): open addressing over 64-bit words (hash high half << 32 | name
// index + 1; 0 = empty), names as (set, id, Clear generation, length, pool offset, hash), bytes in a pool.
// A name is live while its generation equals its set's (a Clear bumps the set's generation).
#pragma once

#include <utility>
#include <vector>

#include "jg_internal.hpp"

namespace jgn {

constexpr uint32_t kNoName = 0xFFFFFFFFu;

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
constexpr uint64_t kFnvBasis = 0xcbf29ce484222325ull, kFnvPrime = 0x100000001b3ull;
// (set, string) key of an element name: the string's FNV-1a mixed with its set and the store's random salt
// (drawn at the store's first wave), so a peer cannot aim names at one value of the sort's low 32 bits
__device__ __forceinline__ uint64_t name_key(uint32_t set, uint64_t fnv, uint64_t salt) {
    return mix64(fnv ^ mix64((uint64_t)set + salt));
}

__device__ __forceinline__ bool same_bytes(const uint8_t* a, const uint8_t* b, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i)
        if (a[i] != b[i]) return false;
    return true;
}

struct Names {
    unsigned long long* tab;
    uint64_t mask;
    uint32_t *set, *id, *gen, *len;
    unsigned long long *off, *key;
    uint8_t* pool;
    uint32_t* set_gen;
    uint32_t* next_id;
    // (set, id) -> name index, for the encoder (jg_orset_encode_json): every name ever issued, dead ones too
    unsigned long long* ikey;  // (set << 32 | id) + 1; 0 = empty
    uint32_t* ival;            // the name's index g
    uint64_t imask;
};

__device__ __forceinline__ void tab_insert(const Names& N, uint64_t key, uint32_t g) {
    const unsigned long long word = (key >> 32) << 32 | (unsigned long long)(g + 1);
    for (uint64_t s = key & N.mask;; s = (s + 1) & N.mask)
        if (atomicCAS(N.tab + s, 0ull, word) == 0ull) return;
}

__device__ __forceinline__ void itab_insert(const Names& N, uint32_t set, uint32_t id, uint32_t g) {
    const unsigned long long k = ((unsigned long long)set << 32 | id) + 1;
    for (uint64_t s = mix64(k) & N.imask;; s = (s + 1) & N.imask)
        if (atomicCAS(N.ikey + s, 0ull, k) == 0ull) {
            N.ival[s] = g;
            return;
        }
}

// The name index of (set, id), or kNoName (a kernel after the inserting ones: no race).
__device__ __forceinline__ uint32_t itab_find(const Names& N, uint32_t set, uint32_t id) {
    const unsigned long long k = ((unsigned long long)set << 32 | id) + 1;
    for (uint64_t s = mix64(k) & N.imask;; s = (s + 1) & N.imask) {
        const unsigned long long w = N.ikey[s];
        if (w == k) return N.ival[s];
        if (w == 0) return kNoName;
    }
}

__device__ __forceinline__ uint32_t tab_find(const Names& N, uint64_t key, uint32_t set, const uint8_t* name, uint32_t len) {
    const uint32_t tag = (uint32_t)(key >> 32), gen = N.set_gen[set];
    for (uint64_t s = key & N.mask;; s = (s + 1) & N.mask) {
        const unsigned long long w = N.tab[s];
        if (w == 0) return kNoName;
        if ((uint32_t)(w >> 32) != tag) continue;
        const uint32_t g = (uint32_t)w - 1;
        if (N.set[g] != set || N.gen[g] != gen || N.len[g] != len || !same_bytes(N.pool + N.off[g], name, len)) continue;
        return N.id[g];
    }
}

}  // namespace jgn

namespace jg {
// The store's element table on the host (orset_names.hip): the buffers Names views, their caps and counts, the names
// log's marks, the range the last commit issued and its page-locked copy.  A member of jg_orset_wire (orset_wave.hpp),
// created empty at the store's first use; growing rebuilds, it changes no content.
struct ElemTable {
    DevBuf tab, nset, nid, ngen, nlen, noff, nkey, pool, set_gen, next_id;
    uint64_t tab_cap = 0, n_names = 0, name_cap = 0, pool_used = 0, pool_cap = 0, set_cap = 0;
    DevBuf ikey, ival;  // (set, id) -> name index (Names::ikey), every name issued
    uint64_t itab_cap = 0;
    // an upper bound of every set's next element id (names_sync's next ids, plus every name a commit issued since);
    // a fast check only: when it would refuse a wave it is first tightened to the exact max (tight_id_bound)
    uint64_t id_bound = 0;
    DevBuf idmax;  // the device max of next_id (tight_id_bound)
    // string-hash mask: all bits; tests narrow it (JANUS_TEST_NAME_HASH_BITS) to force collisions
    uint64_t kmask = ~0ull;
    uint64_t salt = 0;  // name_key's per-store salt (random, drawn at first use)
    // (names held, pool bytes used) after each commit / names_sync: where a names_since pull starts in the pool
    std::vector<std::pair<uint64_t, uint64_t>> marks;
    // ids issued by the last commit: names [g0, g1), pool bytes [p0, p1)
    uint64_t g0 = 0, g1 = 0, p0 = 0, p1 = 0;
    // the names a commit issued, copied into page-locked memory right behind the commit (one queue of copies,
    // no wait): jg_orset_wave_names then waits on `ev` instead of staging them again (~0.6 ms of every
    // ORSetWorkload wave, the host mirror reads them after each wave); layout: jg::NamesStaging
    struct NamesOut {
        uint8_t* host = nullptr;
        size_t cap = 0;
        hipEvent_t ev = nullptr;
        uint64_t g0 = 0, g1 = 0, p0 = 0, p1 = 0;  // what the queued copy holds (g0 == g1: nothing queued)
        // or what stage_now staged: names [since_from, since_to), pool [since_pool0, since_pool1)
        uint64_t since_from = UINT64_MAX, since_to = 0, since_pool0 = 0, since_pool1 = 0, since_bytes = 0;
    } nout;
    std::vector<void*> retired;  // blocks the table outgrew (grow_keep), freed at the next idle point
    ~ElemTable();

    jgn::Names view() const;
    void ensure_sets(jg_ctx* ctx, uint64_t n_sets);
    // Room for `incoming` more names with `pool_bytes` more pool bytes; the table keeps load <= 1/2 (a
    // rebuild keeps live names only).  (0, 0) on a store that never saw a name: empty tables.
    void ensure_names(jg_ctx* ctx, uint64_t incoming, uint64_t pool_bytes);
    uint64_t tight_id_bound(jg_ctx* ctx, DevBuf& cub_temp);
    // n more names hold the log's next indices, the pool is used up to pool_used_now and no set's next id passes
    // next_id_bound: a names_since pull can start here
    void names_added(uint64_t n, uint64_t pool_used_now, uint64_t next_id_bound);
    // A commit issued n_new names (in (set, first entry) order; the check ruled out running past 2^32 - 2): the
    // issued range ends behind them, their page-locked copy is queued and the log marked.
    void issue_names(jg_ctx* ctx, uint64_t n_new, uint64_t pool_used_now);
    void no_names_issued() { g0 = g1 = n_names, p0 = p1 = pool_used; }  // the issued range: empty, at the log's end
};
// orset_wire.hip: the store's table (nullptr while the store has no wire state, unless `create`), and whether a wave
// is open on the store
ElemTable* orset_elem_table(jg_orset* s, bool create);
bool orset_wave_open(const jg_orset* s);
// orset_names.hip: jg_orset_apply_ops_names without its lock and guard (the caller holds the context's lock and
// converts the errors), for update.hip.  Arguments, effects and refusals are that entry point's.  reads: op 4 is allowed,
// Contains of the name at that point of the batch (result[i]): it resolves as a Remove, interns nothing, appends no
// record and moves no ord; a batch of reads only writes neither the store nor the table.
void orset_apply_ops_names_locked(jg_orset* s, uint64_t n_ops, const uint32_t* set, const uint8_t* op, const uint64_t* off, const uint8_t* bytes,
                                  const uint8_t* is_null, const uint64_t* tag_lo, const uint64_t* tag_hi, uint8_t* result, uint32_t* elem_out,
                                  uint64_t* add_lim, uint64_t* rem_lim, bool reads = false);
}  // namespace jg
