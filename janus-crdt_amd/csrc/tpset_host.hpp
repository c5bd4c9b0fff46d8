// tpset_host.hpp — what tpset.hip, tpset_encode.hip and keyspace.hip share on the host: a call's work blocks, the
// count scan, the read of its totals, the offsets check, and the set's bodies the key space calls.  Each function has
// one definition (the unit named beside it); errors are jg::Error, turned into codes by jg::guard at the C ABI only.
#pragma once

#include <array>
#include <cstring>

#include "launch.hpp"
#include "tpset_dict.hpp"

namespace jgt {

// tpset.hip.  At least `bytes` in b (contents lost when it grows; the stream drained first).  The growth policy is
// the set's own, not jg::scratch's.
void* work(jg_ctx* ctx, jg::DevBuf& b, size_t bytes);
// tpset.hip.  out[0..n] = exclusive scan of in[0..n) on the context's stream; block_sums holds the per-block sums of
// a scan past one block's reach.
void excl_scan(jg_ctx* ctx, jg::DevBuf& block_sums, const uint32_t* in, ull* out, uint64_t n);
// tpset.hip.  A batch of strings / messages as (off, bytes): the refusals every entry point shares, named after fn.
void check_offsets(const char* fn, uint64_t n, const uint64_t* off, const uint8_t* bytes);

// Up to four 8-byte totals (the last words of scans) read through the context's page-locked bytes with one sync.
template <class... P> std::array<uint64_t, sizeof...(P)> read_totals(jg_ctx* ctx, const P*... d) {
    static_assert(sizeof...(P) >= 1 && sizeof...(P) <= 4 && ((sizeof(P) == 8) && ...), "one to four 8-byte words");
    size_t at = 0;
    ((jg::pin_get(ctx, at, d, 8), at += 8), ...);
    jg::pin_sync(ctx);
    std::array<uint64_t, sizeof...(P)> v;
    std::memcpy(v.data(), jg::pin_at(ctx, 0), sizeof v);
    return v;
}

// tpset.hip.  The bodies of jg_tpset_create / _apply_ops / _merge_json under the caller's lock: the key space calls
// these, so a failure inside the set reaches jg_keyspace_*'s guard as the jg::Error it was thrown as.
jg_tpset* tpset_create(jg_ctx* ctx, uint64_t cap_strings, uint64_t cap_bytes);
void tpset_apply_ops(jg_tpset* s, uint64_t n, const uint8_t* op, const uint64_t* off, const uint8_t* bytes, const uint8_t* is_null, uint8_t* result);
void tpset_merge_json(jg_tpset* s, uint64_t n, const uint64_t* off, const uint8_t* bytes, uint32_t mode, uint64_t* bad_msg, uint8_t* partial);

// tpset_encode.hip.  Bytes of the encoder's LDS window (jg_tpset_stats.stage_bytes).
uint32_t encode_stage_bytes();

}  // namespace jgt
