// table_hash.hpp — the hashes of the node's two open-addressing tables and the shard rule built on one of them.
// No HIP, no library: plain C++ that device code (through jg_internal.hpp) and a CPU program (host/test_table_hash.cpp)
// compile alike.  Both hashes are bijections on 64 bits (xorshifts and odd multiplies; uid_hash for a fixed hi), so a
// test can invert them and choose the slot a key homes to (tests/node_hash.py).
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JG_HASH_FN __host__ __device__ __forceinline__
#else
#define JG_HASH_FN inline
#endif

namespace jg {

// The node's uid table (uid_table.hpp, node.hip): the home slot of key uid (lo, hi) is uid_hash & mask.
JG_HASH_FN uint64_t uid_hash(uint64_t lo, uint64_t hi) {
    uint64_t x = lo ^ (hi * 0x9E3779B97F4A7C15ull);
    x ^= x >> 31;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 29;
    return x;
}
// The one owner rule of a sharded node (jg_internal.hpp): bits the table's low-bit slot index does not use first.
JG_HASH_FN uint32_t shard_of_uid(uint64_t lo, uint64_t hi, uint32_t world) {
    return world <= 1 ? 0u : (uint32_t)((uid_hash(lo, hi) >> 7) % world);
}
// The safe-update tracker (node.hip): the home slot of a message identity is seq_hash & mask.
JG_HASH_FN uint64_t seq_hash(uint64_t x) {
    x ^= x >> 33;
    x *= 0xFF51AFD7ED558CCDull;
    x ^= x >> 33;
    x *= 0xC4CEB9FE1A85EC53ull;
    return x ^ (x >> 33);
}

}  // namespace jg
