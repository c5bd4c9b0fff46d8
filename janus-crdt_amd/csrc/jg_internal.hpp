// jg_internal.hpp — shared internals of libjanusgpu (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "janus_gpu.h"
#include "orset_walk_small.hpp"
#include "table_hash.hpp"

namespace jgk {  // orset_union.hpp
struct View;
struct Drop;
}

namespace jg {

// Row / set id of a message of another kind in a node wave (csrc/node.hip): the PN-Counter and OR-Set
// passes run over the same uploaded wave and skip each other's messages.
constexpr uint32_t kSkipIdx = 0xFFFFFFFFu;
// Replicas per key the replica table holds (pnc_wire.hpp: per-vector duplicate masks are 4 x 64 bits).
constexpr uint32_t kMaxTableReplicas = 256;

// ---- the one owner rule of a sharded node -------------------
// A key uid belongs to rank shard_of_uid(uid, world) (the apply loop's shard shortcut, jg_shard_of); its
// global key (PN-Counter row / OR-Set set id in the node's key space) is local x world + owner
// (jg_global_key), so the exchange's routing rule owner_of_key(global) = global % world (route.hip, comm.hip)
// names the same rank, and the owner stores it as local key global / world.
// (uid_hash and shard_of_uid: table_hash.hpp, which a CPU program compiles too.)
__host__ __device__ __forceinline__ uint32_t owner_of_key(uint64_t global_key, uint32_t world) { return (uint32_t)(global_key % world); }
__host__ __device__ __forceinline__ uint64_t local_of_key(uint64_t global_key, uint32_t world) { return global_key / world; }

// ---- errors ------------------------------------------------------------------------------------
void set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
void clear_error();

struct Error {  // thrown inside the library only; converted to a code at the ABI edge
    int code;
    std::string msg;
};

[[noreturn]] void fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define JG_HIP(call)                                                                            \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) ::jg::fail(JG_EHIP, "%s failed: %s (%s:%d)", #call,               \
                                        hipGetErrorString(e_), __FILE__, __LINE__);             \
    } while (0)

#define JG_REQUIRE(cond, code, ...) \
    do { if (!(cond)) ::jg::fail((code), __VA_ARGS__); } while (0)

// Run `body` and translate any library error / bad_alloc into an ABI return code.
template <class F> int guard(F&& body) {
    try {
        clear_error();
        body();
        return JG_OK;
    } catch (const Error& e) {
        set_error("%s", e.msg.c_str());
        return e.code;
    } catch (const std::bad_alloc&) {
        set_error("host allocation failed");
        return JG_ENOMEM;
    } catch (...) {
        set_error("unexpected C++ exception");
        return JG_EINVAL;
    }
}

// ---- device buffers ------------------------------------------------------------------------------
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    bool own = true;       // false: a view into another DevBuf's block (never freed through this one)
    void alloc(size_t n);  // frees the old block; n == 0 leaves p null
    void view(void* q, size_t n) {  // a non-owning view (the owner frees the block)
        release();
        p = q;
        bytes = n;
        own = false;
    }
    void release();
    ~DevBuf() { release(); }
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    template <class T> T* as() const { return static_cast<T*>(p); }
};

}  // namespace jg

struct jg_pnc;
namespace jg {
// pnc_dense.hip: a dense identity merge of n_rows device rows into the store (async on the store's stream): the one
// writer of P / N that does not go through rw_P / rw_N, and the one function that advances the shadow's state.
// narrow: the batch is an int64 batch's 4-byte codes (jg_rows).
void pnc_merge_dense(jg_pnc* p, const void* BP, const void* BN, uint64_t n_rows, bool narrow);

// The dense merge's shadow of an int64 store: sP / sN = clamp32 of every cell of P / N, int32
// [n_keys x R], a cache the dense identity merge reads instead of P / N.  cold: no valid shadow (the buffers may be
// kept); armed: the last write to the store was a dense identity merge; valid: the shadow is exact.  Host state under
// the context lock; launches are stream-ordered, so a state set here holds for every later launch.  No file but
// pnc_dense.hip reads the buffers.
struct DenseShadow {
    enum State : uint8_t { kCold = 0, kArmed = 1, kValid = 2 };
    DevBuf sP, sN;
    bool on = true;      // jg_pnc_set_dense_filter
    bool nomem = false;  // the shadow did not fit on the device at this shape: not asked for again until it changes
    State state() const { return state_; }
    void invalidate() { state_ = kCold; }  // another writer has P / N (jg_pnc::rw_P / rw_N)
    void drop();                           // the buffers go too: the store's shape changed, or the filter was set off
    bool ready(size_t bytes);              // the buffers hold `bytes` each (false: no room on the device)

private:
    friend void pnc_merge_dense(jg_pnc*, const void*, const void*, uint64_t, bool);
    State state_ = kCold;
};

// The wave of PNCounterMsg payloads a store is decoding and merging (json.hip): host state under the context lock.
// json.hip is its only writer; other files may only ask is_open().
struct PncWave {
    DevBuf bytes, off, rows;  // an open streamed wave (jg_pnc_wave_*): payload, offsets, rows
    DevBuf stat;              // status words, pass A's deferred marks, pass C's roll-back slots (pnc_wave_layout.hpp)
    DevBuf emit, guid, slow;  // pass A's record per message, the deferred records' Guids, the messages pass B parses again
    uint64_t n = 0, nb = 0;   // messages and bytes appended to the streamed wave; n alone: a node wave's capacity
    uint64_t scan_hi = 0;     // messages pass A scanned since the wave began (its fused applies are undone below this)
    bool open = false;        // between jg_pnc_wave_begin and _commit / _abort
    bool fuse = true;         // the wave's pass A applies what it proves (JANUS_JSON_FUSE, latched when the wave begins)
    bool status_clean = false;  // the status words hold their initial values (the last wave ended clean): no reset
    bool is_open() const { return open; }
};
}  // namespace jg

// ---- handle types (opaque at the ABI) ------------------------------------------------------------
struct jg_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int num_cus = 256;
    jg::DevBuf scratch;  // reusable per-call device scratch (key indices, query keys, staging)
    jg::DevBuf scratch2;
    jg::DevBuf scratch3;
    jg::DevBuf scratch_u;  // update.hip's batch: it outlives the OR-Set side of the call, which uses the three above
    jg::DevBuf flags;   // small zero-initialised status words (error flags)
    // page-locked bytes for small status reads and writes (a pageable copy is staged by the runtime: a blit
    // kernel plus a host copy, ~30-40 us of host gap per round trip): reads at [0, kPinRead), writes from
    // kPinRead (jg::pin_get / pin_sync / pin_at)
    void* hstat = nullptr;
    hipStream_t copy = nullptr;    // wave uploads: chunk k+1's H2D overlaps chunk k's parse on `stream`
    hipEvent_t copied = nullptr;
    // pipelined digests (jg_waves_update_digests): wave k's second-level chains run on `side` while
    // `level1` runs wave k+1's first level, on disjoint CU sets (queue CU masks: a chain that shares its
    // SIMDs with k_sha_msgs waves slows by a quarter); chain_free[s] / level1_done[s] guard the two
    // scratch slots, `begun` orders both after the work already queued on `stream`
    hipStream_t side = nullptr, level1 = nullptr;
    bool cu_masked = false;  // side / level1 hold disjoint CU sets (false: plain streams sharing every CU)
    hipEvent_t level1_done[2] = {nullptr, nullptr}, chain_free[2] = {nullptr, nullptr}, begun = nullptr;
    // Every entry point that reaches this context holds `mu` for the call: the scratch buffers and the
    // streams are shared by all of the context's handles, so concurrent callers (the reference's
    // receiver threads merging prospective copies, readers querying) are serialised here.  Recursive:
    // one-shot entry points reuse the streamed ones on the same thread.
    std::recursive_mutex mu;
};

struct jg_pnc {
    jg_ctx* ctx;
    uint64_t n_keys;
    uint32_t R;
    uint32_t eb;  // elem bytes (4 | 8)
    uint32_t max_R = 0;  // jg_pnc_set_max_replicas: a row-capacity failure widens R up to this (0: fixed shape)
    // The counters, [n_keys x R] of eb bytes each.  Reached through the accessors only: ro_P / ro_N for launches and
    // copies that read, rw_P / rw_N for everything that may write, which invalidates the dense merge's shadow.
    // The dense merge itself (pnc_dense.hip), which keeps the shadow exact, is the one user of the raw fields.
    jg::DevBuf P_, N_;
    const void* ro_P() const { return P_.p; }
    const void* ro_N() const { return N_.p; }
    void* rw_P() { shadow.invalidate(); return P_.p; }
    void* rw_N() { shadow.invalidate(); return N_.p; }
    jg::DenseShadow shadow;  // eb == 8 only
    // replica table (pnc_table.hpp): [n_keys x R] 16-byte Guids + [n_keys] column counts, first use only
    jg::DevBuf cols, ncols;
    // grouped indexed merge (k_group_*): per-key list head of the batch being merged (gen << 32 | row,
    // generation-tagged: no reset between calls) and a next[] link per received row; first use
    jg::DevBuf head, next;
    unsigned long long head_gen = 0;  // generation of the last grouped batch (heads hold gen << 32 | row)
    jg::PncWave wave;        // the wave of state messages in flight (json.hip)
    bool node_open = false;  // a node wave (node.hip) holds the store: see jg::require_writable
};

// Device-resident wave of encoded state messages (json.hip jg_wave_*; digest.hip reads it too).
struct jg_wave {
    jg_ctx* ctx;
    uint64_t cap_msgs, cap_bytes;
    uint64_t n = 0, n_bytes = 0;
    uint32_t max_key = 0;
    jg::DevBuf bytes, off, keys;
};

struct jg_rows {
    jg_ctx* ctx;
    uint64_t n_rows;
    uint32_t R;
    uint32_t eb;
    bool has_keys = false;
    uint32_t max_key = 0;  // largest key_idx uploaded (validated against the store at merge)
    // The received cells, [n_rows x R], in one of two forms.  Wide: eb bytes each, over the whole of P_ /
    // N_.  Narrow (eb == 8 identity batches whose every cell fits, pnc_filter.hpp `fits`): 4-byte codes in the lower
    // half of P_ / N_; the upper half is free (the upload's staging area).  The dense merge (pnc_dense.hip) reads either
    // form in place through the raw fields; every other reader takes the arrays from jg::rows_wide, which widens a
    // narrow batch first.  `narrow` is host state under the context lock; launches are stream-ordered.
    jg::DevBuf P_, N_, keys;
    mutable bool narrow = false;
    bool narrow_on = true;  // jg_rows_set_narrow
    bool may_narrow() const { return eb == 8 && !has_keys && narrow_on; }  // an upload or synth of fitting cells is narrow
};

// One sorted tag-record stream in the CHUNKED layout (orset_union.hpp): structure of arrays
// key[slot] (8 B), tag[slot] (16 B) and ord[slot] (4 B, the arrival ordinal: jg_tagrec.ord); chunk c
// holds ranks [off[c], off[c+1]) in slots [c*kChunk, c*kChunk + cnt[c]); lut[q] = the last chunk
// starting at or before rank q*512.
constexpr uint32_t kChunk = 3072;  // = one union tile (orset.hip kOB * kItems)
struct jg_stream_soa {
    jg::DevBuf block;          // one device block holding the six arrays below (views into it): one hipMalloc and
                               // one hipFree per reservation (hipFree costs ~0.2 ms of host time each on the box)
    jg::DevBuf key, tag, ord;  // cap_chunks * kChunk slots
    uint64_t next = 0;         // every record's ord < next (host copy; a union's B records land at next + ord)
    jg::DevBuf cnt;       // uint32 [cap_chunks]
    jg::DevBuf off;       // uint64 [cap_chunks + 1]
    jg::DevBuf lut;       // uint32 [(cap_chunks * kChunk >> 9) + 2]
    uint64_t cap_chunks = 0;
    uint64_t n = 0;       // records (host copy; see jg_orset::counts_pending)
    uint32_t nch = 0;     // chunks in use
    bool dense = true;    // chunks full except the last (slot = rank): uploads and generated streams
    void reserve_records(uint64_t records);  // room for a dense stream or a union output of `records`
    void swap(jg_stream_soa& o);
    std::vector<void*> retired;  // blocks of earlier reservations (reserve_records), freed at the next idle point
    void free_retired();         // hipFree them (the caller's streams have drained)
    jg_stream_soa() = default;
    jg_stream_soa(const jg_stream_soa&) = delete;
    jg_stream_soa& operator=(const jg_stream_soa&) = delete;
    ~jg_stream_soa();
};

struct jg_orset_wire;  // orset_wave.hpp: element table + open payload wave (first use only)
namespace jg {
void orset_wire_free(jg_orset_wire* w);
void orset_wire_free_retired(jg_orset_wire* w);
}

namespace jg {
int orset_walk_default();  // orset_walk.hip: JANUS_ORSET_WALK = host | device | auto, read once (0 | 1 | 2; unset: 2)
int orset_walk_small_default();  // orset_walk_small.hip: JANUS_ORSET_WALK_SMALL = off | on | auto, read once (0 | 1 | 2; unset: 2)
void orset_walk_small_free(jg_orset* batch);
}

struct jg_orset {
    jg_ctx* ctx;
    // the record walk of Add / Remove / Clear batches (jg_orset_set_walk): 0 on the host (orset.hip
    // apply_ops), 1 on the device (orset_walk.hip), 2 auto; walk_stats: batches walked on the device, on the host, ops
    // walked on the device, bytes of stored runs copied to the host by walks; walk_ws*: the device walk's blocks
    int walk_mode = jg::orset_walk_default();
    uint64_t walk_stats[4] = {0, 0, 0, 0};
    jg::DevBuf walk_ws, walk_ws2, walk_ws3, walk_tmp;
    // the one-launch form of the device walk for small batches (jg_orset_set_walk_small): 0 off, 1 on, 2
    // auto; walk_small_stats: batches walked in one launch, their ops, batches over the stored-tag budget that went to the
    // multi-launch form; walk_small_ws: its fixed scratch, walk_small_batch: its two record streams at their caps (both
    // allocated at the first such batch), walk_small_drop: a Clear drop bitmap of at most 1 MiB
    int walk_small_mode = jg::orset_walk_small_default();
    uint64_t walk_small_stats[3] = {0, 0, 0};
    jg::DevBuf walk_small_ws, walk_small_drop;
    jg_orset* walk_small_batch = nullptr;
    jg_stream_soa add, rem;
    jg_stream_soa spare_add, spare_rem;  // union target for in-place merges (swapped in)
    jg::DevBuf counts;     // device-side uint64 [2]: n_add, n_rem written by the union kernel
    bool counts_pending = false;  // an async union wrote `counts`; host n's are stale
    jg_orset_wire* wire = nullptr;
    bool node_open = false;  // a node wave (node.hip) holds the store: see jg::require_writable
    jg_orset() = default;
    jg_orset(const jg_orset&) = delete;
    jg_orset& operator=(const jg_orset&) = delete;
    ~jg_orset() {
        jg::orset_wire_free(wire);
        jg::orset_walk_small_free(walk_small_batch);
    }
};

namespace jg {
using CtxLock = std::unique_lock<std::recursive_mutex>;
inline CtxLock lock(jg_ctx* c) { return c ? CtxLock(c->mu) : CtxLock(); }
constexpr size_t kPinRead = 32 << 10, kPinBytes = 64 << 10;
// Queue a small device -> host read into the context's page-locked bytes at `at` (< kPinRead); several reads
// share one pin_sync, then pin_at reads them.  Calls on a context are serialised (ctx->mu), and every reader
// syncs before it returns, so the bytes are free at the start of each call.
inline void pin_get(jg_ctx* ctx, size_t at, const void* d, size_t n) {
    if (at + n > kPinRead) fail(JG_EINVAL, "pin_get: %zu bytes at %zu exceed the page-locked read area", n, at);
    JG_HIP(hipMemcpyAsync(static_cast<char*>(ctx->hstat) + at, d, n, hipMemcpyDeviceToHost, ctx->stream));
}
inline void pin_sync(jg_ctx* ctx) { JG_HIP(hipStreamSynchronize(ctx->stream)); }  // (polling measured no gain)
inline const void* pin_at(jg_ctx* ctx, size_t at) { return static_cast<const char*>(ctx->hstat) + at; }
template <class H> inline CtxLock lock(const H* h) { return lock(h ? h->ctx : nullptr); }
// A node wave (node.hip) holds its stores from its begin to its end: the PN-Counter store's wave scratch and
// fused pass A's undo records, the OR-Set store's wave tables (whose element-table lookups assume the committed
// names do not change until the commit).  The one-call form runs under the context lock, but the streamed form
// (jg_apply_stream_begin / _append / _end) keeps the wave open across unlocked calls, so every call that writes
// a store, or reuses the scratch its open wave holds, is refused until the wave ends.
template <class S> inline void require_writable(const S* s, const char* fn) {
    JG_REQUIRE(!s || !s->node_open, JG_EINVAL, "%s: a node wave (jg_apply_stream_begin .. _end) holds this store", fn);
}
inline void check_store(const jg_pnc* p, const char* fn) { JG_REQUIRE(p, JG_EINVAL, "%s: store is NULL", fn); }
void ensure_device(jg_ctx* ctx);  // hipSetDevice(ctx->device) on the calling thread
void* scratch(jg_ctx* ctx, DevBuf& b, size_t bytes);
// After H2D copies queued on ctx->copy: make ctx->stream wait for them (stream order for the kernels
// that read the uploaded chunk).  Callers keep the copy stream off buffers the compute stream may still
// use: before a wave's first upload they record an event at the compute stream's tail (after every setup
// launch of the wave) and make ctx->copy wait on it on the device (node.hip `drained`; the one-shot
// jg_*_wave_append paths synchronise ctx->stream instead), and they synchronise ctx->copy before
// reallocating an upload target (grow_keep) — the same rule covers the D2H copies of issued OR-Set names
// that a commit queues on ctx->copy.
void upload_done(jg_ctx* ctx);
void sync_counts(jg_orset* s);   // fold a pending async count into the host copy
// Dense chunk metadata for a stream whose n records sit contiguously in slots [0, n) (async).
void set_dense(jg_ctx* ctx, jg_stream_soa& s, uint64_t n);
// pnc.hip: scatter-max of n_rows device rows into the store's keys (async on the store's stream).
void pnc_merge_indexed(jg_pnc* p, const void* BP, const void* BN, const uint32_t* d_keys, uint64_t n_rows);
// pnc_dense.hip: the batch's P and N as arrays of eb-byte cells for every reader but the dense merge.  A narrow batch is
// widened in place first (queued on the context's stream) and is wide from then on.
struct WideRows { const void *P, *N; };
WideRows rows_wide(const jg_rows* r);
// pnc.hip: the store grown to at least [n_keys x n_replicas] (jg_pnc_reserve without its open-wave refusals), and
// one doubling of R under jg_pnc_set_max_replicas' bound (false: at the bound).
void pnc_grow(jg_pnc* p, uint64_t n_keys, uint32_t n_replicas);
bool pnc_auto_widen(jg_pnc* p);
// json.hip: the store's replica table, allocated on first use (pnc_table.hpp): [n_keys x R] 16-byte Guids (lo, hi) and
// [n_keys] column counts.  For adopt.hip, which interns a created row's own replica.
struct PncTable { unsigned long long* cols; uint32_t* ncols; uint32_t R; };
PncTable pnc_replica_table(jg_pnc* p);
// pnc.hip: jg_pnc_values' kernel over n device rows (d_keys NULL: rows 0..n), queued on the store's stream.  d_at /
// d_count (query.hip): answer q into slot d_at[q], for the first *d_count rows only; an overflow is written as of_code.
void pnc_values_device(jg_pnc* p, const uint32_t* d_keys, uint64_t n, long long* d_out, uint8_t* d_ovf, const uint32_t* d_at,
                       const unsigned long long* d_count, uint8_t of_code);
// pnc.hip: the same in the middle of a batch (jg_node_exec_keys): read q is command d_at[q] on row d_keys[q], and the
// cell at column col counts as cell - d_dp[d_at[q]] (P) / cell - d_dn[d_at[q]] (N), wrapping at the width: the per-command
// rewinds PncSnap keeps in pdp / pdn.  Queued in front of the batch's adds.
void pnc_values_at_device(jg_pnc* p, uint32_t col, const uint32_t* d_keys, uint64_t n, const long long* d_dp, const long long* d_dn, long long* d_out,
                          uint8_t* d_ovf, const uint32_t* d_at, const unsigned long long* d_count, uint8_t of_code);
// pnc.hip: jg_pnc_apply_ops' wrapping atomic adds over a device list (update.hip): entry i adds d_amount[i] to P (or N
// where d_is_n[i]) at (d_row[i], col), for the first min(*d_count, n_max) entries; queued on the store's stream.  The
// rows are the caller's to check; the column is checked here.  Writes through rw_P / rw_N.
void pnc_add_list_device(jg_pnc* p, const uint32_t* d_row, const long long* d_amount, const uint8_t* d_is_n, const unsigned long long* d_count,
                         uint64_t n_max, uint32_t col);
// orset.hip: merge n_runs sorted, duplicate-free runs (device SoA, run after run) into the store.
void orset_merge_runs(jg_orset* s, uint32_t n_runs, const uint64_t* add_counts, const uint64_t* rem_counts, const unsigned long long* add_key,
                      const uint4* add_tag, const uint32_t* add_ord, const unsigned long long* rem_key, const uint4* rem_tag,
                      const uint32_t* rem_ord);
// orset.hip: largest ord + 1 of n device ords (0 if n == 0), synchronous.
uint64_t ord_span(jg_ctx* ctx, const uint32_t* ord, uint64_t n);
// orset.hip: s = s ∪ src (both streams), src's streams may be dense or chunked; synchronous (the union's error
// flag and counts read back) unless `defer`: then the counts stay pending for orset_pin_pending / _settle.
void orset_merge_store(jg_orset* s, jg_orset* src, bool defer = false);
// orset.hip: a deferred union's error flag and counts queued into the context's page-locked bytes at [at, at
// + 24) (no sync: the caller's own pin_sync brings them with its words; false if nothing is pending), and
// taken from there after that sync (the flag raised as the synchronous merge would).
bool orset_pin_pending(jg_orset* s, size_t at);
// hipFree the blocks the store's streams and element table retired while growing (the caller's streams drained)
void orset_free_retired(jg_orset* s);
// jg_orset_encode_json's first step: every record of the sets d_sets[0..n) (device), query by query, add side then
// tombstones, in store order (element id, tag), into `buf` (grown as needed): key, tag, ord, query << 1 | side, and
// keep = ord below d_lim[q << 1 | side] (d_lim NULL: every record).  roff: [2n + 1] segment offsets.  One round trip.
struct OrsetGathered {
    uint64_t R;
    unsigned long long *key, *tlo, *thi, *roff;
    uint32_t *ord, *qs;
    uint8_t* keep;
};
OrsetGathered orset_gather_sets(jg_orset* s, uint64_t n, const uint32_t* d_sets, const unsigned long long* d_lim, jg::DevBuf& buf);
// orset_encode.hip: what the encoder's write phase needs of its size phase (views into jg_orset_wire::enc and ::enc_g),
// kept on the store's wire state from one to the other.
struct OrsetEncPlan {
    uint64_t n = 0;
    OrsetGathered G{};
    uint32_t *kidx = nullptr, *rid = nullptr, *rstart = nullptr, *srun = nullptr, *rrank = nullptr, *sfirst = nullptr, *srec = nullptr;
    unsigned long long *K = nullptr, *nruns = nullptr, *skey = nullptr, *tlen = nullptr, *rpos = nullptr, *cpos = nullptr, *qsec = nullptr, *qoff = nullptr,
                       *rtags = nullptr;
    unsigned* err = nullptr;
};
// jg_orset_encode_json's size phase over n host set ids at the given ord limits (both NULL: every record), one state per
// entry: h_off [n + 1] on the host, the same offsets left on the device (orset_encode_offsets).  false: a record names an
// element id without a name (h_off is then not a state's length).  Synchronous; nothing is written.  Then its write
// phase at those offsets into d_out (device, h_off[n] bytes), queued on the context's stream.  The caller holds the lock.
bool orset_encode_size_locked(jg_orset* s, uint64_t n, const uint32_t* set, const uint64_t* add_lim, const uint64_t* rem_lim, uint64_t* h_off);
void orset_encode_write_locked(jg_orset* s, uint8_t* d_out);
void orset_settle_pending(jg_orset* s, size_t at);
// The record walk on the device (orset_walk.hip): apply_ops()' contract over the same host arrays, the store's counts
// current.  In auto mode a batch goes there from kWalkAutoMinOps ops on: the smallest measured size at which it is not
// slower than the host walk (host/bench_walk.cpp, DESIGN.md §18: 0.33 / 0.34 ms against 0.09 / 0.10 ms at 1 / 64 ops —
// some forty launches and two waits whatever the size — 0.45 against 0.56 ms at 4096, 1.4 against 7.3 ms at 200,000).
constexpr uint64_t kWalkAutoMinOps = 4096;
void orset_walk_device(jg_orset* s, uint64_t n_ops, const uint32_t* set, const uint32_t* elem, const uint8_t* op, const uint64_t* tag_lo,
                       const uint64_t* tag_hi, uint8_t* result, uint64_t* add_lim, uint64_t* rem_lim);
// orset.hip, for the device walk: a stream's read view, and s = (s minus the sets flagged in `drop`) ∪ batch, synchronous;
// *base_a / *base_r = the store's next ords the batch's records were appended at (read after any renumbering).
jgk::View orset_view(const jg_stream_soa& s);
// The same walk in one launch of one workgroup (orset_walk_small.hip) for a batch of at most
// kWalkSmallMaxOps ops whose Removes and reads name at most kWalkSmallMaxStored stored add tags.  false: the batch
// needs more stored tags than that; nothing has been written and the caller runs orset_walk_device.  In auto mode
// (jg_orset_set_walk 2 with jg_orset_set_walk_small 2) a batch below kWalkAutoMinOps goes there from
// kWalkSmallAutoMinOps ops on: the smallest measured size from which it is not slower than the host walk beyond the
// A/A spread at every larger measured size up to the cap (host/bench_walk.cpp).
constexpr uint64_t kWalkSmallMaxOps = jgs::kMaxOps, kWalkSmallMaxStored = jgs::kMaxStored;
// Measured: 0.14-0.15 ms against the host walk's 0.09-0.10 ms at 1 op and 0.11-0.12 ms at 64 ops (missed), 0.14-0.15
// against 0.15-0.16 ms at 256 ops and 0.16 against 0.25 ms at 1024 ops on ORSetWorkload (met; the Add/Remove mix is
// met from 64 ops on).
constexpr uint64_t kWalkSmallAutoMinOps = 256;
bool orset_walk_small(jg_orset* s, uint64_t n_ops, const uint32_t* set, const uint32_t* elem, const uint8_t* op, const uint64_t* tag_lo,
                      const uint64_t* tag_hi, uint8_t* result, uint64_t* add_lim, uint64_t* rem_lim);
void orset_walk_union(jg_orset* s, jg_orset* batch, jgk::Drop drop, uint64_t* base_a, uint64_t* base_r);
// orset.hip: room in the store's union targets for that many more records (no sync; skipped while counts are pending).
void orset_reserve_union(jg_orset* s, uint64_t add_in, uint64_t rem_in);
// orset.hip, for orset_names.hip: jg_orset_contains' kernel over n device queries (set << 32 | id); jg_orset_lookup_all's
// passes over n device set ids (d_out NULL: member counts into d_cnt_off, else members at the offsets there), both
// queued on the context's stream; and the record side of jg_orset_apply_ops(_ords) over host ids (add_lim / rem_lim
// both or neither), synchronous.
// d_at / d_count / d_out64 (query.hip): answer i into slot d_at[i] of d_out64, for the first *d_count queries only.
void orset_contains_device(jg_orset* s, const unsigned long long* d_q, uint64_t n, uint8_t* d_out, const uint32_t* d_at = nullptr,
                           const unsigned long long* d_count = nullptr, long long* d_out64 = nullptr);
void orset_lookup_all_device(jg_orset* s, const uint32_t* d_set, uint64_t n, uint64_t* d_cnt_off, uint32_t* d_out);
void orset_apply_ops_ids(jg_orset* s, uint64_t n_ops, const uint32_t* set, const uint32_t* elem, const uint8_t* op, const uint64_t* tag_lo,
                         const uint64_t* tag_hi, uint8_t* result, uint64_t* add_lim, uint64_t* rem_lim);

// Node waves (node.hip): one upload of every kind's messages; rows / mset = the message's row / set id
// or kSkipIdx.  json.hip (PN-Counter):
void pnc_node_begin(jg_pnc* p, uint64_t n);
void pnc_node_scan(jg_pnc* p, const uint8_t* bytes, const uint64_t* off, const uint32_t* rows, uint64_t m0, uint64_t m1);
int pnc_node_finish(jg_pnc* p, const uint8_t* bytes, const uint64_t* off, const uint32_t* rows, uint64_t n, uint64_t* bad, std::string* why);
int pnc_node_prefix(jg_pnc* p, const uint8_t* bytes, const uint64_t* off, const uint32_t* rows, uint64_t n, uint64_t* bad, std::string* why);
void pnc_node_undo(jg_pnc* p, const uint32_t* rows);
// SHA-256 of n device-resident payloads into host out (n * 32 bytes), queued on ctx->stream (digest.hip)
// d_null (or NULL): payloads whose flag is set hash to 32 zero bytes
void sha256_device(jg_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, uint8_t* out, const uint8_t* d_null = nullptr);
// pnc_encode.hip, for update.hip (jg_node_update_keys_encode): the snapshots SafeCRDT.Update ships for a
// batch resolved on the device, in two steps with the caller's OR-Set side between them.  The caller holds the
// context's lock and owns the arrays (ctx->scratch_u: they outlive the OR-Set side, which uses the other three).
struct PncSnap {
    // in, one entry per command, in batch order
    const uint32_t* row;      // the command's row; the store's n_keys for a command that applies no PN-Counter op
    const long long* amount;  // its amount (0 for those)
    const uint8_t* is_n;      // 0 = Increment | 1 = Decrement
    const uint8_t* snap;      // 0 none | 1 this command's | 2 the row's latest of the 2s (NULL: 1 everywhere)
    // out
    uint8_t* none;                 // [n] 1: the command ships no snapshot
    unsigned long long* snap_off;  // [n + 1] the commands' byte offsets
    // the encode list: the m commands that ship one, in batch order
    uint32_t* erow;                // [n]
    long long *edp, *edn;          // [n] the row's rewind to the state right after the command (k_encode subtracts it)
    unsigned long long* eoff;      // [n + 1] the list's byte offsets
    // NULL, or [n] each (jg_node_exec_keys): every command's own rewind by command index, kept for the batch's reads;
    // with NULL they are temporaries of the plan
    long long *pdp = nullptr, *pdn = nullptr;
    template <class L> void carve(L& l, uint64_t n, bool keep_prefixes = false) {
        l.add(none, n), l.add(snap_off, n + 1), l.add(erow, n), l.add(edp, n), l.add(edn, n), l.add(eoff, n + 1);
        if (keep_prefixes) l.add(pdp, n), l.add(pdn, n);
    }
};
// Step 1 reads only: per-row prefixes, the survivors of snap == 2, the encode list and its length pass.  Returns with
// m (the list's length) and h_snap_off [n + 1] on the host: two waits on the stream (m sizes the length pass's grid),
// which also cover what the caller queued before it.
// Step 2 queues the write pass into ctx->scratch2, the hashes (sha: n x 32 host bytes or NULL) and the copy to `out`;
// the caller queues the adds behind it and syncs.
// ev (or NULL; JANUS_TRACE_UPDATE): five events of the caller's, recorded behind the prefixes, survivors and list [0] and
// the length pass with the offsets [1] (step 1), the write pass [2], the hashes [3] and the copy of the bytes [4] (step 2).
void pnc_snap_plan_locked(jg_pnc* p, const PncSnap& s, uint64_t n, uint32_t col, uint64_t* m, uint64_t* h_snap_off, hipEvent_t* ev = nullptr);
// Step 2's write pass alone (jg_node_update_keys_ship): the list's bytes in ctx->scratch2, at s.eoff, queued.
const uint8_t* pnc_snap_bytes_locked(jg_pnc* p, const PncSnap& s, uint64_t m, uint64_t bytes, uint32_t col);
// The survivors rule (snap_survivors.hpp) over any object key, for jg_node_update_keys_ship's OR-Set commands: d_obj[i]
// is command i's object (none_obj: it touches none), d_snap as PncSnap::snap; d_none[i] = 1: it ships nothing.  Queued;
// uses ctx->scratch and ctx->scratch3.
void snap_survivors_locked(jg_ctx* ctx, const uint32_t* d_obj, uint64_t n, uint32_t none_obj, const uint8_t* d_snap, uint8_t* d_none);
void pnc_snap_write_locked(jg_pnc* p, const PncSnap& s, uint64_t n, uint64_t m, uint64_t bytes, uint32_t col, uint8_t* out, uint8_t* sha,
                           hipEvent_t* ev = nullptr);
// orset_wire.hip (OR-Set):
void orset_node_begin(jg_orset* s, uint8_t* bytes, uint64_t* off, uint32_t* mset, uint64_t n, uint64_t nbytes, uint32_t max_set);
void orset_node_parse(jg_orset* s, uint64_t m0, uint64_t m1);
int orset_node_check(jg_orset* s, uint64_t n, uint64_t nbytes, uint64_t* bad, std::string* why);
void orset_node_commit(jg_orset* s, uint64_t limit);
void orset_node_abort(jg_orset* s);
void orset_node_no_names(jg_orset* s);
}  // namespace jg
