// tpset_dict.hpp — the resident TPSet<string?> and the key-space dictionary as kernels see them, with their probes:
// shared by tpset.hip and keyspace.hip (which own, fill and grow the set and the dictionary), tpset_encode.hip, query.hip
// and update.hip (which only read them).  One definition of the string hash: a lookup that hashed differently from the
// inserts would find nothing.  Also the call-wide "first index wins" table both owners resolve a call's duplicates in.
#pragma once

#include "jg_internal.hpp"

namespace jgt {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kNullId = 0xFFFFFFFEu;  // the null element's id in add[] / rem[]
constexpr uint32_t kBlock = 256;           // lanes per workgroup of every kernel of the set and the key space
constexpr uint64_t kFnvBasis = 0xcbf29ce484222325ull, kFnvPrime = 0x100000001b3ull;
using ull = unsigned long long;

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// the table key of a string: its FNV-1a mixed with the store's random salt (as name_key in orset_wire.hip), so a
// peer cannot aim strings at one probe run.  The test build keeps 4 bits: every lookup walks long collision runs.
__host__ __device__ __forceinline__ uint64_t str_key(uint64_t fnv, uint64_t salt) {
    const uint64_t k = mix64(fnv ^ salt);
#ifdef JANUS_TEST_HOOKS
    return k & 15;
#else
    return k;
#endif
}

// ---- the resident store as the kernels see it ---------------------------------------------------
struct Store {
    uint8_t* pool;
    ull* soff;
    uint32_t *slen, *sadd, *srem;
    ull* skey;
    uint32_t* table;  // string id + 1, 0 = empty
    uint64_t tmask;
    uint32_t *add, *rem;
    uint32_t* nulls;  // [0] the null element's ordinal in add[], [1] in rem[] (kNone = absent)
    uint64_t salt;
};

__device__ __forceinline__ uint64_t umin(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ bool same_bytes(const uint8_t* a, const uint8_t* b, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i)
        if (a[i] != b[i]) return false;
    return true;
}

// string id of (key, bytes) in the resident table, kNone if absent
__device__ inline uint32_t store_find(const Store& S, uint64_t key, const uint8_t* s, uint32_t len) {
    for (uint64_t slot = key & S.tmask;; slot = (slot + 1) & S.tmask) {
        const uint32_t v = S.table[slot];
        if (v == 0) return kNone;
        const uint32_t id = v - 1;
        if (S.skey[id] == key && S.slen[id] == len && same_bytes(S.pool + S.soff[id], s, len)) return id;
    }
}

// ---- the keySpaces dictionary: an entry holds no bytes of its own (keyspace.hip, jg_keyspace) -------
struct Dict {
    uint32_t* table;  // dictionary id + 1, 0 = empty
    uint64_t mask;
    uint32_t *sid, *klen;
    ull *glo, *ghi, *key;
};

__device__ __forceinline__ ull key_hash(const uint8_t* s, uint32_t n, uint64_t salt) {
    uint64_t h = kFnvBasis;
    for (uint32_t i = 0; i < n; ++i) h = (h ^ s[i]) * kFnvPrime;
    return str_key(h, salt);
}
__device__ inline uint32_t dict_find(const Store& S, const Dict& D, ull key, const uint8_t* k, uint32_t klen) {
    for (uint64_t slot = key & D.mask;; slot = (slot + 1) & D.mask) {
        const uint32_t v = D.table[slot];
        if (v == 0) return kNone;
        const uint32_t d = v - 1;
        if (D.key[d] == key && D.klen[d] == klen && same_bytes(S.pool + S.soff[D.sid[d]], k, klen)) return d;
    }
}

// ---- the call-wide table: one slot per distinct string among a call's items -----------------------
// prep[slot] = a representative item holding the slot's string, + 1 (0 = empty); same(o) = item o's string equals the
// one looked for; key = its table key.  The callers take an atomicMin of the item index per slot, so the first item
// of each distinct string wins.
// claim_slot: the slot of item i's string, claimed for i if no item holds it yet.  A lost CAS is answered by the value
// it returned, never by waiting: the slot then holds some item's string, equal to this one or not.
template <class Same> __device__ __forceinline__ uint32_t claim_slot(uint32_t* prep, uint64_t pmask, ull key, uint32_t i, Same same) {
    for (uint64_t slot = key & pmask;; slot = (slot + 1) & pmask) {
        uint32_t r = prep[slot];
        if (r == 0) {
            r = atomicCAS(&prep[slot], 0u, i + 1);
            if (r == 0) return (uint32_t)slot;
        }
        if (same(r - 1)) return (uint32_t)slot;
    }
}
// find_slot: the same walk once the table only is read; kNone if no item claimed the string
template <class Same> __device__ __forceinline__ uint32_t find_slot(const uint32_t* prep, uint64_t pmask, ull key, Same same) {
    for (uint64_t slot = key & pmask;; slot = (slot + 1) & pmask) {
        const uint32_t r = prep[slot];
        if (r == 0) return kNone;
        if (same(r - 1)) return (uint32_t)slot;
    }
}

}  // namespace jgt

struct jg_tpset {
    jg_ctx* ctx;
    uint64_t cap_strings, cap_bytes;
    uint64_t n_str = 0, n_add = 0, n_rem = 0, n_bytes = 0;
    uint64_t salt = 0, tmask = 0;
    jg::DevBuf pool, soff, slen, sadd, srem, skey, table, add, rem, nulls;
    jg::DevBuf w1, w2, w3;  // work blocks of a call: sized by its messages / elements / candidates
    jg::DevBuf wscan;       // block sums of the long scans
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    jg_tpset_stats stats{};
    double encode_s = 0;  // device seconds of the last encode that wrote (length pass, scan, write pass)
    jgt::Store view() const {
        return jgt::Store{pool.as<uint8_t>(), soff.as<jgt::ull>(), slen.as<uint32_t>(), sadd.as<uint32_t>(), srem.as<uint32_t>(), skey.as<jgt::ull>(),
                          table.as<uint32_t>(), tmask, add.as<uint32_t>(), rem.as<uint32_t>(), nulls.as<uint32_t>(), salt};
    }
    ~jg_tpset() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

struct jg_keyspace {
    jg_ctx* ctx;
    jg_tpset* set = nullptr;
    uint64_t cap = 0, n_keys = 0, jn = 0, seen = 0;  // seen: add ordinals below it went through an OnNext
    jg::DevBuf table, dsid, dklen, dglo, dghi, dkey, jsid, jlen, jglo, jghi, jstatus, wk;
    uint64_t mask = 0;
    jgt::Dict dict() const {
        return jgt::Dict{table.as<uint32_t>(), mask, dsid.as<uint32_t>(), dklen.as<uint32_t>(), dglo.as<jgt::ull>(), dghi.as<jgt::ull>(), dkey.as<jgt::ull>()};
    }
};
