// orset_names.hpp — the OR-Set element table's layout and probes, shared by the wave path (orset_wire.hip, which
// owns and grows the table) and the by-name entry points (orset_names.hip).
//
// Element table (per store, first use): open addressing over 64-bit words (hash high half << 32 | name
// index + 1; 0 = empty), names as (set, id, Clear generation, length, pool offset, hash), bytes in a pool.
// A name is live while its generation equals its set's (a Clear bumps the set's generation).
#pragma once

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
// orset_wire.hip, for orset_names.hip.  The store's element table (created empty at first use) with room for
// n_sets set ids, `incoming` more names and `pool_bytes` more pool bytes; growing rebuilds, it changes no content.
struct NamesRef {
    jgn::Names N;
    uint64_t kmask, salt;         // name_key's mask (tests narrow it) and per-store salt
    uint64_t n_names, pool_used;  // names in the log, pool bytes in use
    uint64_t set_cap;             // sets set_gen / next_id hold
    bool open;                    // a wave is open on the store
};
NamesRef orset_names_ref(jg_orset* s, uint64_t n_sets, uint64_t incoming, uint64_t pool_bytes);
// n names / nb pool bytes were appended behind n_names / pool_used (in log order) by kernels queued on the
// context's stream, which the caller has synchronised; next ids grew to at most id_bound
void orset_names_appended(jg_orset* s, uint64_t n, uint64_t nb, uint64_t id_bound);
}  // namespace jg
