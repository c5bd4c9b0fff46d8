/* janus_gpu.h — C ABI of the MI355X (gfx950) CRDT state-merge engine.
 *
 * Drop-in boundary for the Janus state-merge hot path.  The C#/.NET host binds
 * these with [DllImport("janusgpu")]; tests bind them with ctypes.  Rules:
 *   - extern "C", cdecl, blittable types only (uint8_t instead of bool, no structs with references);
 *   - every pointer argument is caller-owned HOST memory, read or written only during the call;
 *     device memory is library-owned and freed by the matching *_destroy;
 *   - every call returns JG_OK or an error code; the message is in jg_last_error (thread-local);
 *     no exception or abort crosses the ABI;
 *   - calls are synchronous (return after the work is complete) unless they take `async` != 0,
 *     in which case jg_fence(ctx) waits for them;
 *   - thread-safe per context: every call holds its context's lock for its duration (the context's
 *     scratch buffers and HIP stream are shared by all of its handles), so concurrent callers — the
 *     reference's receiver threads merging prospective copies under lock(crdt), readers querying —
 *     are serialised per context; use one context per thread for parallel device work.  Each context
 *     owns one HIP stream (plus a copy stream for wave uploads) on one device.
 *
 * Reference interfaces each entry point replaces are cited per function (paths relative to the
 * reference root, MSRG/Janus-CRDT @ 2025-03-10).
 */
#ifndef JANUS_GPU_H
#define JANUS_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JG_ABI_VERSION 10

/* Error codes.  The C# layer maps them to the exceptions the reference throws (B1 "Errors"). */
#define JG_OK        0
#define JG_EINVAL    1  /* bad argument (ArgumentException / KeyNotFoundException)            */
#define JG_ENOMEM    2  /* device or host allocation failed (OutOfMemoryException)           */
#define JG_EOVERFLOW 3  /* PNCounter.Get checked Sum overflowed (OverflowException)          */
#define JG_ETYPE     4  /* message of the wrong CRDT type (NotSupportedException, ORSet.cs:290) */
#define JG_EHIP      5  /* HIP runtime error                                                  */
#define JG_ESTATE    6  /* precondition broken: unsorted / duplicate records, capacity, timeout */

/* elem id of the C# null element of an ORSet<string?> (ORSet.cs:136-140, nullAddGuid/nullRemoveGuid). */
#define JG_NULL_ELEM 0xFFFFFFFFu

typedef struct jg_ctx jg_ctx;     /* one device + one HIP stream                               */
typedef struct jg_pnc jg_pnc;     /* PN-Counter store: P and N, [n_keys x n_replicas] row-major */
typedef struct jg_rows jg_rows;   /* device-resident batch of received PN-Counter rows          */
typedef struct jg_orset jg_orset; /* OR-Set store: sorted add and tombstone tag records         */

/* One OR-Set tag record: key = (uint64_t)set << 32 | elem, tag = 16 opaque bytes (a C# Guid:
 * tag_lo = bytes 0..7, tag_hi = bytes 8..15, little-endian).  Streams are sorted strictly
 * increasing by (key, tag_lo, tag_hi), unsigned.
 * ord = the record's ARRIVAL ORDINAL, which carries the reference's enumeration order: a HashSet<Guid>
 * enumerates in first-insertion order (ORSet.cs:138-149 Add, :165/178/259/272/281 UnionWith, :182/263/276
 * the copy constructor; nothing removes a single tag), so the tags of one (set, elem) in one stream
 * enumerate in ascending (ord, tag_lo, tag_hi), and a removeSet Dictionary enumerates its elements in
 * ascending (min ord of the element's tombstones, elem) — the element's first insertion.  The addSet
 * Dictionary enumerates in ascending elem id (ids are interned at first insertion).  Only the relative
 * order of ords within one stream of one set is meaningful: the engine renumbers them (order kept) and
 * returns its own values; input ords must be < 2^32.  32 bytes, 8-byte aligned. */
typedef struct jg_tagrec {
    uint64_t key;
    uint64_t tag_lo;
    uint64_t tag_hi;
    uint64_t ord;
} jg_tagrec;

/* ---------------------------------------------------------------------------------------------
 * Context
 * ------------------------------------------------------------------------------------------- */
int jg_abi_version(void);
/* Open device `device` (HIP ordinal) with a private non-blocking stream. */
int jg_open(int device, jg_ctx** out);
int jg_close(jg_ctx* ctx);
/* Copy the calling thread's last error message (NUL-terminated, truncated to n). */
int jg_last_error(char* buf, size_t n);
/* Wait for every async call issued on ctx. */
int jg_fence(jg_ctx* ctx);
/* The context's hipStream_t (for host-side event timing). */
int jg_stream(jg_ctx* ctx, void** hip_stream);

/* ---------------------------------------------------------------------------------------------
 * PN-Counter store — replaces PNCounter's Dictionary<Guid,int> P/N vectors
 * (MergeSharp/MergeSharp/CRDTs/PNCounters.cs:56-153) for a whole keyspace at once.
 * Row = key (host-interned key Guid -> key_idx), column = replica (per-key replica Guid -> column,
 * assigned in first-insertion order so column order = the Dictionary's enumeration order).
 * elem_bytes 4 = the reference's int; 8 = the long variant of BASELINE.json.
 * In RECEIVED rows the most negative value of the width (INT32_MIN / INT64_MIN) means "replica
 * absent from the message": Merge only visits entries the message holds (PNCounters.cs:133-143).
 * ------------------------------------------------------------------------------------------- */
int jg_pnc_create(jg_ctx* ctx, uint64_t n_keys, uint32_t n_replicas, uint32_t elem_bytes, jg_pnc** out);
int jg_pnc_destroy(jg_pnc* pnc);
/* Overwrite rows (key_idx NULL = rows 0..n_rows-1).  Initial load / restore. */
int jg_pnc_write_rows(jg_pnc* pnc, const uint32_t* key_idx, uint64_t n_rows, const void* P, const void* N);
/* Snapshot rows to the host: GetLastSynchronizedUpdate (PNCounters.cs:115-118). */
int jg_pnc_read_rows(jg_pnc* pnc, const uint32_t* key_idx, uint64_t n_rows, void* P, void* N);
/* Merge received states: for each row m and column c whose value is not ABSENT,
 * A[key_idx[m]][c] = max(A[key_idx[m]][c], B[m][c]) for P and N — PNCounter.Merge
 * (PNCounters.cs:131-144) reached through ApplySynchronizedUpdate (:121-125), SafeCRDT.ApplyUpdateStable
 * (BFT-CRDT/SafeCRDTs/SafeCRDT.cs:80-83) and the committed-batch loop
 * (BFT-CRDT/CRDTManagers/SafeCRDTManager.cs:122-146).  key_idx may repeat (the result is the same
 * in any order: max is associative, commutative, idempotent).  key_idx NULL = identity. */
int jg_pnc_merge_rows(jg_pnc* pnc, const uint32_t* key_idx, uint64_t n_rows, const void* P, const void* N);
/* Increment / Decrement (PNCounters.cs:97-112, unchecked '+='): cell (key[i], col[i]) of P
 * (is_n[i] == 0) or N (is_n[i] != 0) += delta[i], wrapping at the store's width. */
int jg_pnc_apply_ops(jg_pnc* pnc, uint64_t n_ops, const uint32_t* key, const uint32_t* col,
                     const int64_t* delta, const uint8_t* is_n);
/* PNCounter.Get (PNCounters.cs:87-90) per key: checked Sum(P) - checked Sum(N), the sums taken in
 * column order, the subtraction wrapping at the store's width.  overflow[i] = 1 (and out[i] = 0)
 * where a checked Sum throws; the call still returns JG_OK.  key_idx NULL = keys 0..n-1. */
int jg_pnc_values(jg_pnc* pnc, const uint32_t* key_idx, uint64_t n, int64_t* out, uint8_t* overflow);

/* The store's current shape (any output may be NULL).  It changes only through jg_pnc_reserve and the
 * widening jg_pnc_set_max_replicas allows. */
int jg_pnc_shape(jg_pnc* pnc, uint64_t* n_keys, uint32_t* n_replicas, uint32_t* elem_bytes);
/* Grow the store in place, on the device, to at least n_keys x n_replicas.  It stands in for what the
 * reference gets for free: a PNCounter's Dictionary<Guid,int> takes any number of replicas as Merge meets
 * them (PNCounters.cs:131-144), and KeySpaceManager.CreateNewKVPair (KeySpaceManager.cs:121-136) creates a
 * key whenever one is learnt.  Never shrinks: a request at or below the current shape in both dimensions
 * returns JG_OK and does nothing.  Afterwards every old cell (k, c) of P and N holds its value and every
 * new cell is 0 (= absent); if the replica table exists, every old slot keeps its Guid, a new key has no
 * columns and every new slot is all-zero; if it does not exist yet it is created at first use, at the new
 * shape.  Refused, the store untouched: n_keys > 2^32 - 1 or n_replicas > 2^30 - 1 (JG_EINVAL);
 * n_replicas > 256 while the replica table exists (JG_EINVAL); a jg_pnc_wave_begin wave is open or a node
 * wave holds the store (JG_EINVAL); an allocation fails (JG_ENOMEM).  The old and the new buffers are
 * resident together during the call (every new buffer is allocated before anything is copied): the device
 * needs room for both.  The call waits for everything queued on the context (an async jg_pnc_merge_batch
 * included) before it releases the old buffers.  A jg_rows batch created for the old n_replicas keeps being
 * refused by jg_pnc_merge_batch: create the batches of the new shape. */
int jg_pnc_reserve(jg_pnc* pnc, uint64_t n_keys, uint32_t n_replicas);
/* Opt-in automatic widening (the same Dictionary growth, PNCounters.cs:131-144; a node whose keys arrive
 * through KeySpaceManager.cs:121-136 cannot know their replicas in advance).  0, the default = a fixed
 * shape: a state naming more replicas than the store's columns fails with JG_ESTATE as ever.  With
 * max_replicas > n_replicas, a jg_pnc_merge_json / _merge_wave / _wave_commit, a jg_pnc_intern or a node
 * wave (jg_apply_committed, jg_apply_block, jg_apply_stream_end) that would fail for row capacity is
 * rolled back as ever, the store widened to min(2 x n_replicas, max_replicas) (and at most the replica
 * table's 256) and the call run again, until it succeeds or the bound is reached.  At the bound the call
 * fails exactly as a fixed store's: same code, same *bad_msg, contents rolled back; the store may stay
 * wider than it was, its contents then the earlier ones padded with zeros.  The caller's bound matters: it
 * is what keeps one faulty peer, naming ever new replicas, from inflating every row of the store.  Keys
 * never grow by themselves: an out-of-range key_idx stays the caller's error.  Read the shape back with
 * jg_pnc_shape after a call that may have widened. */
int jg_pnc_set_max_replicas(jg_pnc* pnc, uint32_t max_replicas);

/* Device-resident received batch (the committed state messages of a wave, decoded to rows).
 * key_idx NULL at upload = identity rows (requires n_rows == the store's n_keys at merge time). */
int jg_rows_create(jg_ctx* ctx, uint64_t n_rows, uint32_t n_replicas, uint32_t elem_bytes, jg_rows** out);
int jg_rows_destroy(jg_rows* rows);
int jg_rows_upload(jg_rows* rows, const uint32_t* key_idx, const void* P, const void* N);
int jg_pnc_merge_batch(jg_pnc* pnc, const jg_rows* rows, int async);
/* The dense merge filter of an int64 store (additive entry points, JG_ABI_VERSION stays 10).  A dense identity
 * merge (jg_pnc_merge_batch of a batch without key indices, jg_pnc_merge_rows with key_idx NULL) needs the
 * store's own cells only to learn whether the received one is larger, and counters overwhelmingly fit 32 bits, so
 * a run of such merges reads a library-private int32 copy of P and N (clamped to the int32 range; a cell at a
 * clamp value is read from the store itself) instead of the 8-byte cells.  The second consecutive dense identity
 * merge with no other write to the store in between allocates and builds the copy (4 more bytes of device memory
 * per cell of P and of N; one more pass of writes in that call), the ones after it read it; any other write to
 * the store (rows, ops, keyed merges, wire-format applies, jg_pnc_reserve, node waves, exchanges) drops it at no
 * cost and the next dense merges start over.  Results are bit-identical with the filter on or off; an int32 store
 * never uses it; if the copy does not fit on the device the store keeps merging without it and returns no error.
 * on != 0 (the default) allows the filter, 0 frees the copy and pins the store to the unfiltered merge (the call
 * waits for the context's queued work first). */
int jg_pnc_set_dense_filter(jg_pnc* pnc, int on);
/* *state = 0: off or cold (no valid copy), 1: armed (the next dense identity merge builds it), 2: valid. */
int jg_pnc_dense_filter_state(jg_pnc* pnc, int* state);
/* The narrow form of a received batch (additive entry points, JG_ABI_VERSION stays 10).  An int64 batch without key
 * indices whose every cell of P and N is ABSENT (INT64_MIN) or in (INT32_MIN, INT32_MAX] is held on the device as
 * 4-byte codes (INT32_MIN for ABSENT, the value otherwise; a real value of INT32_MIN does not fit), and the dense
 * identity merge reads 4 bytes per received cell instead of 8.  The form is decided where the batch is born:
 * jg_rows_upload narrows each chunk as it lands, under the next chunk's copy, and copies the batch again as it is if a
 * cell did not fit; jg_synth_pnc_rows writes the form an upload of the same cells would have.  Batches with key
 * indices and int32 batches are always wide.  No device memory is added (the codes live in the batch's own buffers)
 * and nothing a merge, a route or an exchange returns changes: every reader but the dense merge widens a narrow
 * batch in place first, after which it is wide until its next upload or synth.
 * on != 0 (the default) allows the narrow form; 0 widens a narrow batch now (the call waits for the context's queued
 * work) and pins the batch to the wide form from its next upload or synth on. */
int jg_rows_set_narrow(jg_rows* rows, int on);
/* *form = 0: wide (eb-byte cells), 1: narrow. */
int jg_rows_form(jg_rows* rows, int* form);

/* ---------------------------------------------------------------------------------------------
 * PN-Counter replica table + wire-format apply (csrc/json.hip).  The store keeps, per key, the
 * replica Guids of its columns in first-insertion order (= the stable PNCounter's Dictionary
 * enumeration order, PNCounters.cs:19-25,73-81,131-144); allocated on first use, at most 256
 * replicas per key.  Guids are C# Guid bytes (lo = bytes 0..7, hi = bytes 8..15, little-endian).
 * ------------------------------------------------------------------------------------------- */
typedef struct jg_guid { uint64_t lo, hi; } jg_guid;
typedef struct jg_wave jg_wave;   /* device-resident wave of encoded state messages            */

/* Register replica[i] in row key_idx[i], in order (append if absent); col_out[i] = its column.
 * The PNCounter() constructor's {self: 0} (PNCounters.cs:73-81): CreateSafeCRDT registers the
 * stable instance's own Guid first.  JG_ESTATE (nothing registered) if a row would overflow. */
int jg_pnc_intern(jg_pnc* pnc, uint64_t n, const uint32_t* key_idx, const jg_guid* replica, uint32_t* col_out);
/* Column tables of rows key_idx[0..n): replicas[i*R + c] for c < ncols[i]. */
int jg_pnc_columns(jg_pnc* pnc, uint64_t n, const uint32_t* key_idx, jg_guid* replicas, uint32_t* ncols);
/* Apply a committed wave of PNCounterMsg wire payloads (System.Text.Json UTF-8, PNCounters.cs:38-49):
 * message i = bytes[off[i], off[i+1]) (off[0] = 0) is decoded and merged into row key_idx[i]
 * exactly as SafeCRDT.ApplyUpdateStable (BFT-CRDT/SafeCRDTs/SafeCRDT.cs:80-83) -> Decode -> Merge
 * would, message after message (SafeCRDTManager.cs:122-146); new replicas get columns in commit
 * order.  All or nothing: a message outside the accepted JSON form (oracle/json.hpp) returns
 * JG_EINVAL, a key running out of columns JG_ESTATE, nothing is applied, and *bad_msg (if not NULL)
 * = the first such message (UINT64_MAX on success).  The caller re-submits the prefix
 * [0, *bad_msg) to reproduce the reference, whose loop applies the messages before the throwing one. */
int jg_pnc_merge_json(jg_pnc* pnc, uint64_t n, const uint32_t* key_idx, const uint64_t* off, const uint8_t* bytes, uint64_t* bad_msg);
/* The same call streamed in chunks, so the caller's gathering of chunk k+1 overlaps the upload and the
 * decode/validation pass of chunk k: begin (capacity hints; exceeded capacity grows), append chunks
 * in commit order (chunk offsets relative to the chunk: off[0] = 0; returns once the upload and pass A
 * are queued — the chunk's host buffers must stay untouched until commit or abort returns), then
 * commit (= jg_pnc_merge_json over the concatenation: all or nothing, *bad_msg indexes the whole
 * wave) or abort (nothing applied).  One open wave per store. */
int jg_pnc_wave_begin(jg_pnc* pnc, uint64_t cap_msgs, uint64_t cap_bytes);
int jg_pnc_wave_append(jg_pnc* pnc, uint64_t n, const uint32_t* key_idx, const uint64_t* off, const uint8_t* bytes);
int jg_pnc_wave_commit(jg_pnc* pnc, uint64_t* bad_msg);
int jg_pnc_wave_abort(jg_pnc* pnc);
/* The same with the wave already in device memory (upload once, merge many: the bench). */
int jg_wave_create(jg_ctx* ctx, uint64_t cap_msgs, uint64_t cap_bytes, jg_wave** out);
int jg_wave_destroy(jg_wave* wave);
int jg_wave_upload(jg_wave* wave, uint64_t n, const uint32_t* key_idx, const uint64_t* off, const uint8_t* bytes);
int jg_pnc_merge_wave(jg_pnc* pnc, const jg_wave* wave, uint64_t* bad_msg);

/* GetLastSynchronizedUpdate().Encode() (PNCounters.cs:115-118, 46-49) of rows key_idx[0..n): state i
 * = out[off[i], off[i+1]) (off has n+1 entries, always filled), System.Text.Json's compact form over
 * the row's replica table in column order — what SafeCRDT.Update ships (BFT-CRDT/SafeCRDTs/SafeCRDT.cs:49).
 * out NULL = size query; JG_ESTATE if off[n] > cap (out untouched). */
int jg_pnc_encode_json(jg_pnc* pnc, uint64_t n, const uint32_t* key_idx, uint64_t* off, uint8_t* out, uint64_t cap);
/* The same for the row as it stood before its last dp[i] / dn[i] of Increment / Decrement amounts to column col
 * (the cell type's wrapping arithmetic): the snapshot SafeCRDT.Update shipped right after an earlier op of a
 * batch whose later ops on the same key are already applied (SafeCRDT.cs:39-62; PNCounters.cs:97-112).  Lets a
 * batch of client ops be applied in ONE jg_pnc_apply_ops and every snapshot encoded in ONE call. */
int jg_pnc_encode_json_before(jg_pnc* pnc, uint64_t n, const uint32_t* key_idx, uint32_t col, const int64_t* dp, const int64_t* dn,
                              uint64_t* off, uint8_t* out, uint64_t cap, uint8_t* sha);
/* A round of SafeCRDT.Update's PN-Counter client ops at once (SafeCRDT.cs:39-62; PNCounterWrapper.Update ->
 * Increment / Decrement, PNCounters.cs:96-112, on this copy's own column col): every op applied (as jg_pnc_apply_ops),
 * and for each op with need[i] != 0, in op order, dp / dn = the Increment / Decrement amounts the batch's LATER ops
 * on the same key added (wrapping at the store's width) — the rewind jg_pnc_encode_json_before takes to encode the
 * snapshot that op shipped.  Computed on the device (a sort of the ops by key, newest first, and a segmented sum).
 * dp / dn hold count(need) entries.  ABI v9. */
int jg_pnc_apply_ops_rewind(jg_pnc* pnc, uint64_t n_ops, const uint32_t* key, uint32_t col, const int64_t* delta, const uint8_t* is_n,
                            const uint8_t* need, int64_t* dp, int64_t* dn);
/* The whole PN-Counter round in one call (SafeCRDT.cs:39-62 per op: Increment / Decrement on column col, then
 * GetLastSynchronizedUpdate().Encode()): op i's snapshot — the key's row right after op i, i.e. the row before the
 * batch plus the key's ops 0..i — into out[off[i], off[i+1]) (and its SHA-256 into sha + 32 i when sha is not
 * NULL), then every op applied.  The prefixes are a sort + segmented sum on the device; nothing crosses the host
 * link but the ops, the offsets and the bytes.  JG_ESTATE if off[n] > cap: off filled, NOTHING applied (call
 * again with a larger out).  ABI v10. */
int jg_pnc_apply_ops_encode(jg_pnc* pnc, uint64_t n_ops, const uint32_t* key, uint32_t col, const int64_t* delta, const uint8_t* is_n,
                            uint64_t* off, uint8_t* out, uint64_t cap, uint8_t* sha);
/* (sha, here and in jg_orset_encode_json: NULL, or n * 32 bytes receiving each encoded state's SHA256 — the hash
 * UpdateMessage.ComputeDigest takes of it, DAGUpdateMessage.cs:43 — computed on the device from the bytes just
 * written; filled only when out is.  The producer path feeds them to jg_update_digests_of.) */

/* Page-locked host memory for staging waves (PCIe DMA at full rate); free with jg_host_free. */
int jg_host_alloc(jg_ctx* ctx, uint64_t bytes, void** out);
int jg_host_free(void* p);

/* ---------------------------------------------------------------------------------------------
 * OR-Set store — replaces ORSet<string>'s Dictionary<T,HashSet<Guid>> add/remove maps and null
 * tag sets (MergeSharp/MergeSharp/CRDTs/ORSet.cs:78-327) for a whole keyspace of sets.
 * ------------------------------------------------------------------------------------------- */
int jg_orset_create(jg_ctx* ctx, uint64_t cap_add, uint64_t cap_rem, jg_orset** out);
int jg_orset_destroy(jg_orset* s);
/* Replace the state with the given sorted streams (validated: JG_ESTATE if not strictly increasing). */
int jg_orset_load(jg_orset* s, const jg_tagrec* add, uint64_t n_add, const jg_tagrec* rem, uint64_t n_rem);
int jg_orset_size(jg_orset* s, uint64_t* n_add, uint64_t* n_rem);
/* Canonical snapshot (GetLastSynchronizedUpdate, ORSet.cs:305-308). */
int jg_orset_read(jg_orset* s, jg_tagrec* add, uint64_t cap_add, jg_tagrec* rem, uint64_t cap_rem);
/* ORSet.Merge (ORSet.cs:253-283): per element UnionWith of the add and tombstone tag sets (null
 * element included), from host records (sorted, strictly increasing). */
int jg_orset_merge(jg_orset* s, const jg_tagrec* add, uint64_t n_add, const jg_tagrec* rem, uint64_t n_rem);
/* dst = dst ∪ src for two device-resident stores. */
int jg_orset_merge_store(jg_orset* dst, const jg_orset* src, int async);
/* out = a ∪ b (out must have capacity for a+b; it may not alias a or b). */
int jg_orset_union(const jg_orset* a, const jg_orset* b, jg_orset* out, int async);
/* ORSet.Add / Remove / Clear (ORSet.cs:134-198), the OR-Set ApplyOp, applied in op order per set
 * (ORSetWrapper.Update op ids, BFT-CRDT/SafeCRDTs/ORSetWrapper.cs:30-46): op[i] = 1 Add(elem[i]) with
 * the fresh tag (tag_lo[i], tag_hi[i]) the caller drew (Guid.NewGuid()); 2 Remove(elem[i]) — tombstones
 * every tag of the element's add set if Contains(elem) at that point; 3 Clear() of set[i].
 * result[i] = the op's bool result (Remove: 0 when the element was absent).  Any other op id is
 * JG_EINVAL before anything changes (the wrapper's InvalidOperationException). */
int jg_orset_apply_ops(jg_orset* s, uint64_t n_ops, const uint32_t* set, const uint32_t* elem, const uint8_t* op,
                       const uint64_t* tag_lo, const uint64_t* tag_hi, uint8_t* result);
/* The same, and per op i the ord limits of a snapshot of its set taken right after it (SafeCRDT.Update's
 * GetLastSynchronizedUpdate() after each op, SafeCRDT.cs:39-62): jg_orset_encode_json with add_lim[i] / rem_lim[i]
 * encodes the set as it stood then — valid while no later op of the batch Clears that set (a Clear drops the
 * records such a snapshot holds). */
int jg_orset_apply_ops_ords(jg_orset* s, uint64_t n_ops, const uint32_t* set, const uint32_t* elem, const uint8_t* op, const uint64_t* tag_lo,
                            const uint64_t* tag_hi, uint8_t* result, uint64_t* add_lim, uint64_t* rem_lim);
/* Where a store walks its batches of ORSet.Add / Remove / Clear (ORSet.cs:134-198) (additive entry points,
 * JG_ABI_VERSION stays 10).  Every entry point that applies such ops (jg_orset_apply_ops, _ords, _names, the node's
 * by-key-name calls, the producer path) turns the batch into records, ords and results by one walk in op order:
 * mode 0 replays it on the host over the stored tag runs of every element a Remove or a read names, fetched from the
 * device; mode 1 computes the same with sorts and prefix sums on the device, and no stored run crosses to the host;
 * mode 2 (auto) picks by batch size.  Results, records, ords and limits are bit-identical in every mode.  A new store
 * starts in auto, or in the mode the environment variable JANUS_ORSET_WALK = host | device | auto names (read once).
 * Any other mode is JG_EINVAL. */
int jg_orset_set_walk(jg_orset* s, int mode);
/* The store's walks of ORSet.Add / Remove / Clear batches (ORSet.cs:134-198) since its creation: out[0] batches walked
 * on the device, out[1] on the host, out[2] ops walked on the device, out[3] bytes of stored runs copied to the host
 * by walks. */
int jg_orset_walk_stats(jg_orset* s, uint64_t out[4]);
/* Whether the device walk of an ORSet.Add / Remove / Clear batch (ORSet.cs:134-198) may take its one-launch form
 * (additive entry points, JG_ABI_VERSION stays 10): one kernel launch by one workgroup computes what the multi-launch
 * device walk computes, for a batch of at most out[4] ops of jg_orset_walk_small_stats whose Removes and reads name
 * at most out[5] stored add tags; a batch over that second budget is walked by the multi-launch form instead, never
 * on the host.  Mode 0 is off, 1 on, 2 auto.  Under jg_orset_set_walk mode 0 the switch is ignored; under mode 1 a
 * fitting batch takes the one-launch form iff the switch is on; under mode 2 a batch below the multi-launch form's
 * threshold takes it if the switch is on and the batch fits, or if the switch is auto and the batch's size is in the
 * measured range where the form is not slower than the host walk (from 256 ops up to the cap), and is walked on the
 * host otherwise.  Results, records, ords and limits are bit-identical in every form.  A new store
 * starts in auto, or in the mode the environment variable JANUS_ORSET_WALK_SMALL = off | on | auto names (read
 * once).  Any other mode is JG_EINVAL and changes nothing. */
int jg_orset_set_walk_small(jg_orset* s, int mode);
/* The store's one-launch walks of ORSet.Add / Remove / Clear batches (ORSet.cs:134-198) since its creation: out[0]
 * batches walked in one launch, out[1] their ops, out[2] batches that fit the op cap, exceeded the stored-tag budget
 * and went to the multi-launch walk, out[3] reserved (0), out[4] the op cap, out[5] the stored-tag budget.  A
 * one-launch batch is a device walk: it also counts in jg_orset_walk_stats out[0] and out[2]. */
int jg_orset_walk_small_stats(jg_orset* s, uint64_t out[6]);
/* ORSet.Contains (ORSet.cs:204-237) for (set[i], elem[i]): elem present iff its add set exists
 * and (it has no tombstone set or the two tag sets differ: !SetEquals); the null element is
 * present iff !SetEquals(nullRemove, nullAdd).  out[i] = 0/1. */
int jg_orset_contains(jg_orset* s, const uint32_t* set, const uint32_t* elem, uint64_t n, uint8_t* out);
/* The records of whole sets set[0..n) (every element and null): set i's adds are
 * add[add_off[i], add_off[i+1]), its tombstones rem[rem_off[i], rem_off[i+1]), sorted; the offsets
 * (n+1 entries each) are always filled.  add and rem NULL = size query; JG_ESTATE if a buffer is
 * short.  The per-set GetLastSynchronizedUpdate (ORSet.cs:305-308) that SafeCRDT.Update encodes. */
int jg_orset_read_sets(jg_orset* s, uint64_t n, const uint32_t* set, uint64_t* add_off, jg_tagrec* add, uint64_t cap_add, uint64_t* rem_off,
                       jg_tagrec* rem, uint64_t cap_rem);
/* ORSetMsg.Encode() (MergeSharp/MergeSharp/CRDTs/ORSet.cs:56-69, 305-308) of sets set[0..n) from the device store,
 * byte for byte the reference's System.Text.Json output: addSet elements in ascending element id (= the add
 * Dictionary's insertion order), removeSet elements by their first tombstone's arrival ordinal (ties by id),
 * tags by (ord, tag) (HashSet<Guid> insertion order), the null element's tags in nullAddGuid / nullRemoveGuid;
 * element strings from the store's element table (names issued by waves or synced with jg_orset_names_sync —
 * JG_ESTATE if a record's id has none).  add_lim / rem_lim (both or neither; NULL = everything): state i keeps
 * only its set's add records with ord < add_lim[i] and tombstones with ord < rem_lim[i] — a snapshot taken
 * before a batch's later ops (jg_orset_apply_ops_ords).  State i = out[off[i], off[i+1]); out NULL = size
 * query; JG_ESTATE if off[n] > cap (off filled, out untouched). */
int jg_orset_encode_json(jg_orset* s, uint64_t n, const uint32_t* set, const uint64_t* add_lim, const uint64_t* rem_lim, uint64_t* off,
                         uint8_t* out, uint64_t cap, uint8_t* sha);
/* ORSet.LookupAll (ORSet.cs:204-227) of sets set[0..n): members of set[i] are elems[off[i], off[i+1])
 * (off has n+1 entries, always filled), in the reference's order: elements with no tombstone set,
 * then elements whose tag sets differ (each group in ascending elem id = the add Dictionary's
 * insertion order when elem ids are interned at first insertion), then JG_NULL_ELEM if null is
 * present.  elems NULL = size query; JG_ESTATE if off[n] > cap (nothing written to elems). */
int jg_orset_lookup_all(jg_orset* s, uint64_t n, const uint32_t* set, uint64_t* off, uint32_t* elems, uint64_t cap);

/* ---------------------------------------------------------------------------------------------
 * OR-Set wire-format apply (csrc/orset_wire.hip; SURVEY.md §8f F1 + A7/A13).  ORSetMsg<string>
 * payloads (System.Text.Json UTF-8, ORSet.cs:56-69) decoded, their element strings interned and the
 * states merged on the device, as SafeCRDT.ApplyUpdateStable (BFT-CRDT/SafeCRDTs/SafeCRDT.cs:80-83)
 * -> ORSet.DecodePropagationMessage -> Merge (ORSet.cs:253-283) would, message after message.
 * Element table: per set, element string -> 32-bit element id, ids issued in first-insertion order
 * (the add/remove Dictionaries' order; addSet entries before removeSet within a state, Merge's walk)
 * and never reused; Clear drops a set's live strings (later adds take new ids).  The device table
 * is the wave path's copy of the caller's interning: the caller registers the names it issues itself
 * (ORSet.Add ops) and the Clears it applies with jg_orset_names_sync before the next wave, and reads
 * back the ids a wave issued with jg_orset_wave_names.
 * ------------------------------------------------------------------------------------------- */
/* Register caller-side interning changes, applied in this order: for each i < n_sets, set[i]'s live
 * strings are dropped if cleared[i] and its next id becomes next_id[i]; then name i < n_names
 * (bytes[off[i], off[i+1]), off[0] = 0) is live in set name_set[i] with id name_id[i] (the caller
 * guarantees it is not live already). */
int jg_orset_names_sync(jg_orset* s, uint64_t n_sets, const uint32_t* set, const uint32_t* next_id, const uint8_t* cleared,
                        uint64_t n_names, const uint32_t* name_set, const uint32_t* name_id, const uint64_t* off, const uint8_t* bytes);
/* A committed wave of ORSetMsg payloads, streamed like jg_pnc_wave_*: message i of the wave (chunks in
 * commit order, chunk-relative offsets, off[0] = 0) is the state of set[i].  append uploads a chunk and
 * queues its validation pass (host buffers untouched until commit / abort returns).  check ends the
 * validation (element names repeated inside one map need the whole wave): JG_OK, or the code of the
 * first message the reference's Decode/Merge would throw on — JG_EINVAL (JsonException: not an
 * ORSetMsg in the accepted form of oracle/json.hpp, a null member or tag set, an element repeated in
 * one map) or JG_ESTATE (an element whose add or tombstone tag set is empty: Add always inserts a tag and
 * Remove copies a non-empty add set, so no reference state holds one, and the record layout has no
 * record to carry the Dictionary key it would add) — with *bad_msg = its
 * wave index (UINT64_MAX if none).  commit merges messages [0, limit) (limit <= *bad_msg): interns
 * their new element strings in commit order and unions their tag records into the store; the wave
 * closes.  abort closes the wave with nothing applied. */
int jg_orset_wave_begin(jg_orset* s, uint64_t cap_msgs, uint64_t cap_bytes);
int jg_orset_wave_append(jg_orset* s, uint64_t n, const uint32_t* set, const uint64_t* off, const uint8_t* bytes);
int jg_orset_wave_check(jg_orset* s, uint64_t* bad_msg);
int jg_orset_wave_commit(jg_orset* s, uint64_t limit);
int jg_orset_wave_abort(jg_orset* s);
/* The element ids the last commit issued, sorted by (set, id): name i = bytes[off[i], off[i+1]) got id
 * id[i] in set set[i].  set / id / off / bytes NULL = size query (*n_names, *n_bytes). */
int jg_orset_wave_names(jg_orset* s, uint64_t* n_names, uint64_t* n_bytes, uint32_t* set, uint32_t* id, uint64_t* off, uint8_t* bytes);
/* The store's names log: every name the element table took, in the order it took them (commits and
 * jg_orset_names_sync alike; never reordered, cleared names stay in it).  Names [from, *to) with *to = the
 * log's length now: name i - from = bytes[off[i], off[i+1]) with id id[i] in set set[i] (the caller skips
 * the ones it synced itself).  set / id / off / bytes NULL = size query (*to, *n_bytes).  A caller that only
 * needs the ids when it next interns or reads a name pulls them then, several waves at once, instead of
 * after every wave (jg_orset_wave_names) — the ORSetWorkload wave's ~0.7 ms of host copying leaves the
 * apply loop (replaces nothing in the reference: its names live in the C# Dictionaries, ORSet.cs:83-88). */
int jg_orset_names_since(jg_orset* s, uint64_t from, uint64_t* to, uint64_t* n_bytes, uint32_t* set, uint32_t* id, uint64_t* off, uint8_t* bytes);
/* One-shot: begin + append(all) + check, then commit(n) if every message is good; else nothing is
 * applied and the check's code is returned with *bad_msg (the jg_pnc_merge_json contract). */
int jg_orset_merge_json(jg_orset* s, uint64_t n, const uint32_t* set, const uint64_t* off, const uint8_t* bytes, uint64_t* bad_msg);

/* ---------------------------------------------------------------------------------------------
 * The OR-Set by element name (csrc/orset_names.hip).  ORSet<string>'s members take strings
 * (ORSet.cs:134-237); these calls resolve and intern them in the store's own element table, the one
 * wave commits and jg_orset_names_sync fill, so a caller needs no string <-> id dictionaries.
 * Name arrays as jg_tpset_*: name i = bytes[off[i], off[i+1]) with off[0] = 0, is_null[i] = 1 for the
 * C# null element (its length is ignored).  Names are the element's UTF-8 bytes, unescaped, compared byte
 * for byte, shorter than 2^31; "" is an ordinary element, distinct from null.  A set id the table has never
 * seen is an empty set.  Locking and refusals as the id-taking counterparts.
 * --------------------------------------------------------------------------------------------- */
/* name -> live element id of set[i]: JG_NULL_ELEM for null, JG_NULL_ELEM - 1 ("never allocated", the id no
 * record carries) when the set's live table lacks it.  Read-only.  (Replaces the caller's per-set
 * Dictionary<string, id>; in the reference the strings are the keys of addSet / removeSet, ORSet.cs:83-88.) */
int jg_orset_resolve_names(jg_orset* s, uint64_t n, const uint32_t* set, const uint64_t* off, const uint8_t* bytes,
                           const uint8_t* is_null, uint32_t* elem);
/* ORSet.Contains(item) (ORSet.cs:234-237) by string. */
int jg_orset_contains_names(jg_orset* s, uint64_t n, const uint32_t* set, const uint64_t* off, const uint8_t* bytes,
                            const uint8_t* is_null, uint8_t* out);
/* ORSet.LookupAll() (ORSet.cs:204-227) as strings, in jg_orset_lookup_all's order: members of set[i] are entries
 * [off[i], off[i+1]); entry k = bytes[name_off[k], name_off[k+1]), is_null[k] = 1 for the null element (zero length);
 * elems (optional) = the ids.  off and *n_bytes always filled; name_off/bytes/is_null NULL = size query; JG_ESTATE
 * with nothing written if cap_elems / cap_bytes are short, or if a member's id has no name in the table. */
int jg_orset_lookup_all_names(jg_orset* s, uint64_t n, const uint32_t* set, uint64_t* off, uint64_t* n_bytes,
                              uint64_t* name_off, uint8_t* bytes, uint8_t* is_null, uint32_t* elems,
                              uint64_t cap_elems, uint64_t cap_bytes);
/* ORSet.Add / Remove / Clear by string (ORSet.cs:134-198), op ids and results as jg_orset_apply_ops; the name of a
 * Clear is ignored.  Per set, in op order: an Add takes its name's live id or interns it with the set's next id
 * (ids only grow, also across Clear; several Adds of one new name share the id issued at the first); a Remove takes
 * the id if the name is live at that point, else JG_NULL_ELEM - 1 (result 0, nothing interned); a Clear drops the
 * set's live names.  The new names join the names log (jg_orset_names_since) in the order of their first Add;
 * jg_orset_wave_names is not affected.  elem_out (optional): the id each op addressed (0 for a Clear).
 * add_lim / rem_lim (both or neither): as jg_orset_apply_ops_ords.  All or nothing: JG_EINVAL for an op id other than
 * 1..3, NULL arguments, bad offsets or an open wave, JG_ESTATE for a set out of element ids. */
int jg_orset_apply_ops_names(jg_orset* s, uint64_t n_ops, const uint32_t* set, const uint8_t* op, const uint64_t* off,
                             const uint8_t* bytes, const uint8_t* is_null, const uint64_t* tag_lo, const uint64_t* tag_hi,
                             uint8_t* result, uint32_t* elem_out, uint64_t* add_lim, uint64_t* rem_lim);

/* ---------------------------------------------------------------------------------------------
 * The committed-wave apply loop (csrc/node.hip) — SafeCRDTManager.HandleAfterConsensusUpdates
 * (BFT-CRDT/CRDTManagers/SafeCRDTManager.cs:109-160) as ONE call per committed wave (SURVEY.md §8b B2's
 * jg_apply_batch).  Inside the library: the walk in commit order, the skip of creation and key-space
 * messages (:133-134), the uid lookup safeCRDTsIndexedByuid.TryGetValue (:136) in a device hash table,
 * Decode + Merge of every state (SafeCRDT.ApplyUpdateStable, BFT-CRDT/SafeCRDTs/SafeCRDT.cs:80-83) on the
 * device, and safeUpdateTracker.TryRemove (:141-142) in a device table.  The library's host workers only
 * gather the payloads into page-locked staging, chunk by chunk, while the device parses the chunk before.
 * ------------------------------------------------------------------------------------------- */
typedef struct jg_node jg_node;        /* one copy (stable or prospective) of a node's keyspace          */
typedef struct jg_tracker jg_tracker;  /* SafeCRDTManager.safeUpdateTracker (SafeCRDTManager.cs:33)     */

/* A node's copy of its keys over a PN-Counter store and an OR-Set store of one context (either NULL if the
 * node holds no key of that type).  The stores stay owned by the caller and must outlive the node. */
int jg_node_create(jg_pnc* pnc, jg_orset* orset, jg_node** out);
int jg_node_destroy(jg_node* node);
/* SafeCRDTManager.CreateSafeCRDT (SafeCRDTManager.cs:61-101) -> safeCRDTsIndexedByuid[uid] = sc (:73, :98):
 * key uid[i] is a PNCounter (type 0) at row idx[i] of the node's store, or an ORSet (type 1) at set id
 * idx[i].  All or nothing: JG_EINVAL for Guid.Empty, a uid registered twice, a row >= the store's n_keys,
 * a set id >= 2^31 - 16, or a type whose store the node lacks.  (The PNCounter constructor's own replica
 * column is jg_pnc_intern's, as before.) */
int jg_node_register(jg_node* node, uint64_t n, const jg_guid* uid, const uint8_t* type, const uint32_t* idx);
/* Key-space sharding over the GPUs of a node: the owner rank of a key is
 * jg_shard_of(uid, world) (a hash of the 16 uid bytes).  A node declared shard `rank` of `world` leaves
 * another shard's states out of its gather from the uid alone — no upload, no lookup; the uid table would
 * skip them the same way (:136), since such a node registers only its own keys.  Registering a uid of
 * another shard turns the shortcut off (the table decides every state again); each jg_node_set_shard
 * rescans the registered uids.  world 1 = no sharding. */
int jg_node_set_shard(jg_node* node, uint32_t rank, uint32_t world);
int jg_shard_of(const jg_guid* uid, uint32_t world, uint32_t* rank);

int jg_tracker_create(jg_ctx* ctx, jg_tracker** out);
int jg_tracker_destroy(jg_tracker* t);
/* ConcurrentDictionary.TryAdd of SafeCRDT.Update (BFT-CRDT/SafeCRDTs/SafeCRDT.cs:55-56: a safe update with a
 * client origin): seq[i] (>= 1, < UINT64_MAX) identifies the NetworkProtocol object, origin[i] (!= 0) the
 * (Connection, id) to notify.  Thread-safe without the context lock (the reference's client threads add
 * while the apply task runs) and cheap: buffered, the device table takes the adds at the next call that
 * reads the tracker.  An identity already tracked keeps its entry. */
int jg_tracker_add(jg_tracker* t, uint64_t n, const uint64_t* seq, const uint64_t* origin);
/* Count: the identities tracked, every jg_tracker_add before the call included.  Both reads first move the buffered
 * adds into the device table, unless a streamed wave (jg_apply_stream_begin .. _end) is open on the tracker and they
 * would not fit the table as it stands: that wave classifies against the table it began with and completes into it,
 * so the table is not rebuilt, cleared or freed under it.  The adds then stay buffered until the wave has ended, and
 * both reads answer from the device table plus the buffered pairs (an identity in either is tracked, counted once).
 * An identity added while a wave is open is either completed by that wave or still tracked after it, never both. */
int jg_tracker_size(jg_tracker* t, uint64_t* n);
/* ContainsKey: out[i] = 1 while seq[i] is tracked (see jg_tracker_size for a read while a streamed wave is open). */
int jg_tracker_contains(jg_tracker* t, uint64_t n, const uint64_t* seq, uint8_t* out);

/* A committed wave in commit order (Consensus.Commit's List<List<UpdateMessage>>, Consensus.cs:123-134,
 * flattened: list, block, update): message i is NetworkProtocol{uid[i], syncMsgType type[i]
 * (0 ManagerMsg_Create, 1 CRDTMsg), message} (MergeSharp/MergeSharp/proto/SyncProtocol.cs:12-62) with
 * identity seq[i] (0 = never tracked; seq NULL = all 0).  Payloads either contiguous (off[n + 1], off[0] = 0,
 * bytes) or scattered (off NULL: message i = ptr[i][0 .. len[i])).  Contiguous payloads in page-locked
 * memory (jg_host_alloc) are uploaded from there without a host copy. */
typedef struct jg_commit {
    uint64_t n;
    const jg_guid* uid;
    const uint8_t* type;
    const uint64_t* seq;
    const uint64_t* off;
    const uint8_t* bytes;
    const uint8_t* const* ptr;
    const uint32_t* len;
} jg_commit;

/* HandleAfterConsensusUpdates over one committed wave.  completed[0 .. *n_completed) = the origins of the
 * safe updates the wave completed (their tracker entries removed), in commit order — the
 * safeUpdateCompleteClientNotifier calls; completed needs room for n entries (NULL: count only); tracker
 * may be NULL.  A state its key's Decode / Merge rejects stops the loop there, as the reference's apply
 * Task faults at it: every message before *stopped_at was applied and its completions reported, nothing
 * from it on, and the call returns the rejection's code (JG_EINVAL: JsonException; JG_ESTATE: an OR-Set
 * element with an empty tag set, or a key out of replica columns) — the one entry point that applies a
 * prefix on error.  JG_OK with *stopped_at = UINT64_MAX otherwise.  An internal failure of the wave's OR-Set
 * commit (its device error flag) is returned AFTER the completions: completed / *n_completed are valid,
 * *stopped_at = UINT64_MAX, and the OR-Set store must be reloaded (its union did not finish). */
int jg_apply_committed(jg_node* node, jg_tracker* tracker, const jg_commit* wave, uint64_t* completed, uint64_t* n_completed,
                       uint64_t* stopped_at);
/* ConnectionManager.ReceivedBlock -> ReplicationManager.ReceivedUpdateSyncMsg (BFT-CRDT/Network/DAGConnectionManager.cs:40-50,
 * MergeSharp/MergeSharp/ReplicationManager.cs:290-344) on a node's PROSPECTIVE copy: the same without a
 * tracker; a CRDT state of an uid the node never registered stops the block there with JG_EINVAL
 * (KeyNotFoundException, RM:329).  The shard shortcut does not apply. */
int jg_apply_block(jg_node* node, const jg_commit* wave, uint64_t* stopped_at);
/* jg_apply_committed handed over part by part, so the caller's own copy of the committed byte[]s into page-locked
 * memory overlaps the uploads and parses of the parts before (SafeCRDTManager.cs:109-160 over
 * a wave that arrives block by block).  begin: at most n_max messages and bytes_max payload bytes; append: the next
 * part (commit indices continue from the previous part; a part whose payloads are page-locked and contiguous is
 * uploaded in place, else gathered) — its chunks' uploads and parses are queued before it returns; end: the cut,
 * both commits and the completions, exactly as jg_apply_committed over the concatenated parts.  A part that breaks
 * the wave's rules (decreasing offsets, past the begin's bounds) rejects the whole wave: nothing of it is applied
 * and the stream is closed.  No shard shortcut (every part is uploaded whole).  One streamed wave per node.  A
 * page-locked part's payload bytes are read by the device after append returns: they must stay unchanged until
 * end returns (a gathered part's arrays and every part's uid / type / identity arrays are copied by append). */
int jg_apply_stream_begin(jg_node* node, jg_tracker* tracker, uint64_t n_max, uint64_t bytes_max);
int jg_apply_stream_append(jg_node* node, const jg_commit* part);
int jg_apply_stream_end(jg_node* node, uint64_t* completed, uint64_t* n_completed, uint64_t* stopped_at);
/* Figures of the node's last apply call.  Host: seconds gathering payloads into staging, waiting for the
 * device after the last chunk was queued, the whole call.  Device: kernel time of the wave (hipEvents
 * around each chunk's kernels and around the final phase, on the context's stream) = chunk_busy_s (the
 * per-chunk classify + parse kernels: the payload decode) + tail_busy_s (after the last chunk).  Messages
 * and payload bytes uploaded, messages applied (registered CRDT states before the cut), chunks.  Host
 * phases (ABI v5, appended): setup_s (registrations and tracker adds to the device, buffers sized, the
 * previous call's kernels drained) and loop_s (the chunk loop: gathers + queueing the uploads and kernels);
 * total_s = setup_s + loop_s + device_wait_s + argument checks. */
typedef struct jg_apply_stats {
    double gather_s, device_wait_s, total_s, device_busy_s;
    uint64_t msgs_uploaded, bytes_uploaded, msgs_applied, chunks;
    double chunk_busy_s, tail_busy_s;
    double setup_s, loop_s;
} jg_apply_stats;
int jg_node_last_stats(jg_node* node, jg_apply_stats* out);

/* ---------------------------------------------------------------------------------------------
 * Cross-shard exchange (csrc/route.hip).  The keyspace of a node is sharded over
 * its GPUs: global key k (PN-Counter row / OR-Set set id) belongs to rank k % world, where it is
 * local key k / world.  The reference has one process per node and no sharding: these entry points
 * serve the sharded deployment of the same stores (one process per GPU) when a received batch
 * lands on a rank that does not own all of its keys — the received states still reach
 * PNCounter.Merge (PNCounters.cs:131-144) / ORSet.Merge (ORSet.cs:253-283) on the owner.
 * EXCEPTION to the host-pointer rule above: the d_* arguments are caller-owned DEVICE memory of the
 * context's device (the collective's send / receive buffers, e.g. RCCL all-to-all over xGMI); the
 * library checks that they are device memory of that device and large enough, and returns after
 * its stream is idle.
 * ------------------------------------------------------------------------------------------- */
/* Stable partition of a device batch by owner rank: d_keys[n_rows] (local keys), d_P/d_N[n_rows x R]
 * receive the rows grouped by destination rank in batch order; counts[world] (host) = rows per
 * destination.  world in [1, 64]; cap_rows >= the batch's rows. */
int jg_rows_route(const jg_rows* rows, uint32_t world, uint64_t* counts, void* d_keys, void* d_P, void* d_N, uint64_t cap_rows);
/* jg_pnc_merge_rows from device memory: rows (d_keys[i], d_P[i], d_N[i]), ABSENT cells skipped, keys
 * may repeat; all or nothing (JG_EINVAL if any key >= n_keys, nothing merged). */
int jg_pnc_merge_device(jg_pnc* pnc, uint64_t n_rows, const void* d_keys, const void* d_P, const void* d_N);
/* Stable partition of both record streams of a store by owner rank (set id % world; set ids
 * rewritten to set / world): keys (8 B), tags (16 B, jg_tagrec order) and ords (uint32_t) per stream. */
int jg_orset_route(jg_orset* s, uint32_t world, uint64_t* add_counts, uint64_t* rem_counts, void* d_add_key, void* d_add_tag,
                   void* d_add_ord, uint64_t cap_add, void* d_rem_key, void* d_rem_tag, void* d_rem_ord, uint64_t cap_rem);
/* ORSet.Merge of n_runs received runs (run r = add_counts[r] adds and rem_counts[r] tombstones,
 * stored run after run; each sorted strictly increasing, JG_ESTATE otherwise) into the store, in run
 * order: run r is the r-th state merged (its ords order its own records, jg_tagrec.ord). */
int jg_orset_merge_device(jg_orset* s, uint32_t n_runs, const uint64_t* add_counts, const uint64_t* rem_counts, const void* d_add_key,
                          const void* d_add_tag, const void* d_add_ord, const void* d_rem_key, const void* d_rem_tag, const void* d_rem_ord);

/* The exchange itself, inside the library over RCCL (csrc/comm.hip): one communicator per process (one
 * rank per GPU of the node), then one call per received batch does route -> all-gather of the counts ->
 * grouped ncclSend/ncclRecv of every run over the xGMI peer links (this rank's own run by a device copy)
 * -> merge of the received runs in source-rank order.  Collective: every rank of the communicator makes
 * the same exchange call (a rank with nothing received passes an empty batch / store). */
typedef struct jg_comm jg_comm;
/* ncclGetUniqueId into id[128]: made by one rank and handed to the others over the caller's own channel. */
int jg_comm_unique_id(uint8_t* id);
/* A non-blocking RCCL communicator (ncclCommInitRankConfig, blocking = 0) on ctx's device: returns once all
 * `world` ranks have joined with the same id, or JG_EHIP after JANUS_COMM_TIMEOUT_S seconds (default 120)
 * with the half-made communicator aborted.  Every exchange on it polls against the same deadline: a rank that
 * never posts its half, or an RCCL async error, aborts the communicator and returns JG_EHIP (every later
 * call on it then fails at once) instead of hanging. */
int jg_comm_init(jg_ctx* ctx, uint32_t rank, uint32_t world, const uint8_t* id, jg_comm** out);
/* The host transport: the same exchange with the counts and the runs moved by the caller's all-to-all-v over
 * host memory — send holds the runs for peers 0..world-1 back to back (send_bytes[p] each), recv receives
 * the peers' runs back to back (recv_bytes[p] each, known in advance); returns 0 on success.  For ranks that
 * RCCL cannot serve (several ranks on one GPU, or shards moved over the caller's own links). */
typedef int (*jg_alltoallv_fn)(void* user, const void* send, const uint64_t* send_bytes, void* recv, const uint64_t* recv_bytes);
int jg_comm_init_host(jg_ctx* ctx, uint32_t rank, uint32_t world, jg_alltoallv_fn fn, void* user, jg_comm** out);
int jg_comm_destroy(jg_comm* comm);
/* The exchange's plan (pure host arithmetic, what every exchange call follows): counts[(src * world + dst) * k
 * + j] = records source src routes to destination dst in buffer j (the all-gathered route counts).  For this
 * rank and each peer p, buffer j (index p * k + j): send[send_off .. + send_n) goes to p (the send buffer
 * holds every destination's run in rank order) and recv[recv_off .. + recv_n) comes from p (the peers' runs
 * back to back in source-rank order).  skip_own: the own run is neither sent nor received (the PN-Counter
 * exchange merges it from the send buffer).  world <= 64. */
int jg_exchange_plan(uint32_t rank, uint32_t world, uint32_t k, const uint64_t* counts, uint8_t skip_own, uint64_t* send_off, uint64_t* send_n,
                     uint64_t* recv_off, uint64_t* recv_n);
/* The one owner rule (SafeCRDTManager.cs:136's routing, sharded): a key registered by the rank
 * jg_shard_of(uid, world) names as its owner, with that rank's local index `local`, has the global key
 * local * world + owner — the id the exchange routes by (owner = global % world, local = global / world). */
int jg_global_key(const jg_guid* uid, uint32_t world, uint32_t local, uint32_t* global);
/* PNCounter.Merge (PNCounters.cs:131-144) of a received batch on the owners of its keys: rows is this
 * rank's batch in GLOBAL keys (row key k goes to rank k % world as local key k / world), store this
 * rank's shard (rows NULL: this rank sends nothing).  sent[world] / received[world] (optional): rows per
 * destination / per source. */
int jg_pnc_exchange(jg_comm* comm, jg_pnc* store, const jg_rows* rows, uint64_t* sent, uint64_t* received);
/* ORSet.Merge (ORSet.cs:253-283) of a received state (global set ids: set s goes to rank s % world as
 * s / world) on the owners: the runs merged into store in source-rank order (jg_orset_merge_device).
 * Per-destination / per-source record counts of both streams (optional, world entries each). */
int jg_orset_exchange(jg_comm* comm, jg_orset* store, jg_orset* received, uint64_t* sent_add, uint64_t* sent_rem, uint64_t* recv_add,
                      uint64_t* recv_rem);
/* Figures of the communicator's last exchange: device seconds of route, counts + runs, merge (hipEvents on
 * the context's stream); bytes that left / reached this rank over the links; records merged. */
typedef struct jg_exchange_stats {
    double route_s, exchange_s, merge_s;
    uint64_t bytes_sent, bytes_received, records_received;
} jg_exchange_stats;
int jg_comm_last_stats(jg_comm* comm, jg_exchange_stats* out);

/* ---------------------------------------------------------------------------------------------
 * UpdateMessage digests (csrc/digest.hip) — replaces UpdateMessage.ComputeDigest
 * (BFT-CRDT/DAGConsensus/DAGUpdateMessage.cs:32-55), run by `new UpdateMessage(list)` (:25-30) for
 * every batch the client batcher submits (SafeCRDTManager.ActualPropagateSyncMsg, SafeCRDTManager.cs:165-198).
 * ------------------------------------------------------------------------------------------- */
/* n NetworkProtocol.message payloads: payload i = bytes[off[i], off[i+1]) (off[0] = 0), a C# null when
 * is_null != NULL && is_null[i] (hashed as 32 zero bytes, :41-42).  n_updates UpdateMessages: update u
 * holds payloads [first[u], first[u+1]) (first[0] = 0, first[n_updates] = n).  digest[32u..32u+32) =
 * SHA256(SHA256(payload) for each payload of u ‖ zeros up to ArrayPool<byte>.Shared.Rent(32 * count)
 * .Length) — the .NET 6 bucket length (oracle/digest.hpp).  msg_digest (optional, n * 32 bytes) receives
 * each payload's SHA256 (zeros for null).  Synchronous; JG_EINVAL on malformed offsets. */
int jg_update_digests(jg_ctx* ctx, uint64_t n, const uint64_t* off, const uint8_t* bytes, const uint8_t* is_null, uint64_t n_updates,
                      const uint64_t* first, uint8_t* msg_digest, uint8_t* digest);
/* SHA256.HashData of n payloads (payload i = bytes[off[i], off[i+1]), off[0] = 0) into out (n * 32 bytes): the
 * per-message hashes ComputeDigest takes (DAGUpdateMessage.cs:43), for a caller that assembles UpdateMessages
 * later from payloads it already holds in one buffer (a page-locked `bytes` uploads in place).  Synchronous. */
int jg_sha256_batch(jg_ctx* ctx, uint64_t n, const uint64_t* off, const uint8_t* bytes, uint8_t* out);
/* ComputeDigest's second level from per-payload hashes the caller already has (jg_sha256_batch, or
 * jg_update_digests' msg_digest): msg_digest[32i..32i+32) = SHA256 of payload i (ignored for a null payload,
 * is_null[i] != 0: hashed as 32 zero bytes), update u = payloads [first[u], first[u+1]) as in jg_update_digests.
 * digest[32u..) = the same bytes jg_update_digests gives.  Synchronous. */
int jg_update_digests_of(jg_ctx* ctx, uint64_t n, const uint8_t* msg_digest, const uint8_t* is_null, uint64_t n_updates, const uint64_t* first,
                         uint8_t* digest);
/* The same over a wave already in device memory (jg_wave_upload; no null payloads): first[n_updates]
 * must equal the wave's message count. */
int jg_wave_update_digests(const jg_wave* wave, uint64_t n_updates, const uint64_t* first, uint8_t* msg_digest, uint8_t* digest);
/* The same for n_waves device-resident waves of one context in ONE call, pipelined: wave k+1's
 * per-payload hashes run while wave k's UpdateMessage chains (the serial second level) run on a second
 * stream.  Wave k: n_updates[k] UpdateMessages over payloads first[k][u].. (rules as above, first[k]
 * [n_updates[k]] = that wave's count), digests into digest[k] (n_updates[k] * 32 bytes).  A wave may
 * appear more than once.  Synchronous; JG_EINVAL (nothing computed) when any wave's arguments are
 * malformed or the waves belong to different contexts.  The batched form of the per-batch
 * ComputeDigest calls the batcher makes (SafeCRDTManager.cs:165-198 → DAGUpdateMessage.cs:25-30). */
int jg_waves_update_digests(const jg_wave* const* waves, uint64_t n_waves, const uint64_t* n_updates, const uint64_t* const* first,
                            uint8_t* const* digest);
/* SHA256.HashData of every payload of a device-resident wave (the per-message hashes ComputeDigest takes,
 * DAGUpdateMessage.cs:43) into DEVICE memory d_out (wave count * 32 bytes, digest bytes), for a consumer
 * on the device; async != 0 returns once queued on the context's stream (jg_fence waits). */
int jg_wave_sha256(const jg_wave* wave, void* d_out, uint8_t async);

/* ---------------------------------------------------------------------------------------------
 * Key-space set (csrc/tpset.hip, csrc/tpset_encode.hip) — one TPSet<string?> resident on the device
 * (MergeSharp/MergeSharp/CRDTs/2P-Set.cs:60-213), the CRDT Janus keeps its own key space in
 * (BFT-CRDT/CRDTManagers/KeySpaceManager.cs:34,87: every key as key + "\0" + guid).  Additive to ABI v10: these
 * entry points are new names, nothing existing changes (JG_ABI_VERSION stays 10); jg_apply_committed /
 * jg_apply_block still skip key-space messages, a caller opts in by calling these.
 * Strings are UTF-8 bytes; the C# null element (HashSet<string?> holds it) is carried as a flag.  A string's
 * ORDINAL is its index in addSet's (or removeSet's) enumeration order: nothing is ever removed from either
 * HashSet, so that is first-insertion order.  String batches are (off[n + 1], off[0] = 0, bytes) as elsewhere.
 * ------------------------------------------------------------------------------------------- */
typedef struct jg_tpset jg_tpset;
/* new TPSet<string>() (2P-Set.cs:93-97) with room for cap_strings distinct strings (the null element not
 * counted) of cap_bytes UTF-8 bytes in all. */
int jg_tpset_create(jg_ctx* ctx, uint64_t cap_strings, uint64_t cap_bytes, jg_tpset** out);
int jg_tpset_destroy(jg_tpset* set);
/* addSet.Count, removeSet.Count (Count, 2P-Set.cs:76-82, is *n_add - *n_rem, reported literally even when a
 * merge put strings into removeSet that addSet lacks) and the string bytes held.  Any pointer may be NULL. */
int jg_tpset_size(jg_tpset* set, uint64_t* n_add, uint64_t* n_rem, uint64_t* n_bytes);
/* Add (2P-Set.cs:106-109, op[i] = 1) and Remove (:117-126, op[i] = 2: only if Contains) of string i (the null
 * element where is_null != NULL && is_null[i]), in op order.  result[i] (optional) = 1 for an Add, Remove's bool
 * for a Remove.  Any other op id, or bytes that are not well-formed UTF-8: JG_EINVAL; out of strings or bytes:
 * JG_ESTATE; nothing applied either way. */
int jg_tpset_apply_ops(jg_tpset* set, uint64_t n, const uint8_t* op, const uint64_t* off, const uint8_t* bytes, const uint8_t* is_null,
                       uint8_t* result);
/* Contains (2P-Set.cs:169-172): out[i] = in addSet and not in removeSet. */
int jg_tpset_contains(jg_tpset* set, uint64_t n, const uint64_t* off, const uint8_t* bytes, const uint8_t* is_null, uint8_t* out);
/* LookupAll (2P-Set.cs:133-136): addSet.Except(removeSet) in addSet's order, from add ordinal from_ord on.  Member
 * k: ord[k], bytes[off[k], off[k+1]), is_null[k] = the null element (no bytes).  ord / off / bytes / is_null all
 * NULL = size query (*n members, *n_bytes bytes); else *n / *n_bytes hold the buffers' capacities on entry (off
 * has room for *n + 1) and the sizes on return; JG_ESTATE if a buffer is short (sizes still returned). */
int jg_tpset_lookup_all(jg_tpset* set, uint64_t from_ord, uint64_t* n, uint64_t* n_bytes, uint64_t* ord, uint64_t* off, uint8_t* bytes,
                        uint8_t* is_null);
/* ApplySynchronizedUpdate (2P-Set.cs:195-199) -> TPSetMsg.Decode (:40-46) -> Merge (:188-192) of n encoded
 * states {"addSet":[...],"removeSet":[...]}, message after message: addSet.UnionWith then removeSet.UnionWith, new
 * strings taking ordinals in the arrays' order.  The accepted form is oracle/json.hpp's contract (whitespace,
 * members in any order, unknown members skipped to depth 64, a repeated member's last occurrence, full JSON strings,
 * a string repeated in one array de-duplicated, `null` elements).  One rule differs on purpose from the PN-Counter /
 * OR-Set decoders: Merge walks addSet first, so a message whose addSet is valid but whose removeSet is missing or
 * null has its addSet merged and the call stops there with *partial = 1 (the reference throws between the two
 * UnionWith calls); a message whose addSet is missing or null, or that is malformed anywhere, applies nothing.
 * Every message before the first such message is applied and nothing after it: JG_EINVAL with *bad_msg = its
 * index (UINT64_MAX on success).  JG_ESTATE (out of strings or bytes): nothing applied.
 * mode 0 = automatic: messages in flat form (one object, addSet then removeSet, each once, arrays of strings or
 * nulls, any whitespace) go through the parallel scanner, every other message through the serial parser, which is
 * the definition; mode 1 = the serial parser only.  Both give the same store. */
int jg_tpset_merge_json(jg_tpset* set, uint64_t n, const uint64_t* off, const uint8_t* bytes, uint32_t mode, uint64_t* bad_msg, uint8_t* partial);
/* GetLastSynchronizedUpdate().Encode() (2P-Set.cs:210-213, :49-52) of the whole set, byte for byte System.Text.Json's
 * compact output (strings escaped by JavaScriptEncoder.Default).  out NULL = size query; JG_ESTATE if *n_bytes >
 * cap (out untouched). */
int jg_tpset_encode_json(jg_tpset* set, uint64_t* n_bytes, uint8_t* out, uint64_t cap);
/* Figures of the set's last jg_tpset_merge_json: messages and payload bytes each parser took, array elements the
 * applied messages held (strings_seen), entries appended to addSet or removeSet (strings_new), the scanner's tile
 * size, device seconds (hipEvents around the call's kernels). */
typedef struct jg_tpset_stats {
    uint64_t msgs_parallel, bytes_parallel, msgs_serial, bytes_serial;
    uint64_t strings_seen, strings_new;
    uint64_t tile_bytes;
    double device_s;
    uint64_t stage_bytes; /* the encoder's write pass stages this many wire bytes per window                     */
    double encode_s;      /* device seconds of the set's last jg_tpset_encode_json that wrote: length pass, scan   */
                          /* (one host read of the total between them) and write pass; the copy out excluded      */
} jg_tpset_stats;
int jg_tpset_last_stats(jg_tpset* set, jg_tpset_stats* out);

/* ---------------------------------------------------------------------------------------------
 * Key space (csrc/keyspace.hip) — KeySpaceManager's state on the device (BFT-CRDT/CRDTManagers/KeySpaceManager.cs): the
 * set above, the keySpaces dictionary (key string -> Guid, :30) and the LastKeySpaceSet watermark (:35).  Additive
 * to ABI v10.  Keys are UTF-8 bytes in (off[n + 1], off[0] = 0, bytes) batches; Guids are jg_guid.
 * ------------------------------------------------------------------------------------------- */
typedef struct jg_keyspace jg_keyspace;
/* new KeySpaceManager: room for cap_keys entries of cap_bytes bytes in all (an entry is key + "\0" + 36-byte guid). */
int jg_keyspace_create(jg_ctx* ctx, uint64_t cap_keys, uint64_t cap_bytes, jg_keyspace** out);
int jg_keyspace_destroy(jg_keyspace* ks);
/* The underlying set (owned by the key space), for jg_tpset_encode_json (GetLastSynchronizedUpdate of the key-space
 * CRDT, what CreateNewKVPair ships) and queries.  Merge into it only through jg_keyspace_receive. */
int jg_keyspace_set(jg_keyspace* ks, jg_tpset** set);
/* CreateNewKVPair (KeySpaceManager.cs:121-136) for a batch, in order: keySpaces.TryAdd(key, guid) (:130; added[i] =
 * its bool, optional) and then, whatever it returned, keySpaceCRDT.Add(key + "\0" + guid.ToString()) (:131). */
int jg_keyspace_create_keys(jg_keyspace* ks, uint64_t n, const uint64_t* off, const uint8_t* key_bytes, const jg_guid* guid, uint8_t* added);
/* The key-space CRDT's ApplySynchronizedUpdate followed by OnNext (KeySpaceManager.cs:151-178), message after
 * message (jg_tpset_merge_json's contract per message, mode included; each message is one merge on the device, so
 * many small states in one call cost one round of launches each).  OnNext takes LookupAll().Except(LastKeySpaceSet):
 * an entry is SEEN by the OnNext of the message that added it unless that message or an earlier one put it in
 * removeSet; a removal by a later message does not unsee it.  For each seen entry, in ordinal order and in the
 * reference's order of evaluation (:163-166): key = the bytes before the first NUL (the whole entry if it has none);
 * if the dictionary holds that key - from jg_keyspace_create_keys, an earlier message or an earlier entry of the same
 * OnNext - nothing happens, whatever the rest of the entry looks like; else guid = the segment between the first and
 * the second NUL (Split("\0")[1]) in "D" form of either case, and the key is added with that guid (the first entry
 * wins) and journalled.
 * A message Decode / Merge rejects stops the call as in jg_tpset_merge_json (JG_EINVAL, *bad_msg, *partial; its
 * OnNext does not run: entries a partial merge added are seen by the next message's OnNext).  *n_new = journal
 * records this call appended.  JG_ESTATE from the dictionary or the journal (neither can fill before the set does)
 * comes after that message's merge, which is not rolled back: the watermark stays and the next call's OnNext takes
 * those entries.
 * DEPARTURE (stated, parity-unpinned): the reference throws out of OnNext on an entry without a NUL
 * (IndexOutOfRangeException), with a guid segment Guid.Parse rejects (FormatException) or on the null element (NRE),
 * before LastKeySpaceSet advances, and so wedges on that entry at every later message; Guid.Parse also accepts forms
 * other than "D", which an honest node never writes.  Here such an entry is journalled with a status, not added to
 * the dictionary, and processing goes on; only the "D" form is a guid.  The departure covers only entries on which the
 * reference throws: a NUL-less or bad-guid entry of a key the dictionary holds is skipped there and here alike; one of
 * an unknown key adds nothing, so a later well-formed entry of that key still wins; the null element is dereferenced
 * before any lookup and is journalled (status 3) whatever the dictionary holds. */
int jg_keyspace_receive(jg_keyspace* ks, uint64_t n, const uint64_t* off, const uint8_t* bytes, uint32_t mode, uint64_t* bad_msg, uint8_t* partial,
                        uint64_t* n_new);
/* The journal of OnNext's outcomes since record `from`, in the style of jg_orset_names_since: records [from, *to)
 * with *to = the journal's length now; record i - from = bytes[off[i], off[i+1]), guid[i], status[i]: 0 = key added
 * (bytes = the key); 1 = the entry has no NUL; 2 = its guid segment is not in "D" form; 3 = the null element (1-3:
 * bytes = the raw entry, guid zero, nothing added; 1 and 2 only for a key the dictionary lacked at that entry).  off / bytes / guid / status all NULL = size query (*to,
 * *n_bytes); else *n_bytes holds bytes' capacity on entry (JG_ESTATE if short) and off has *to - from + 1 entries. */
int jg_keyspace_new_keys(jg_keyspace* ks, uint64_t from, uint64_t* to, uint64_t* n_bytes, uint64_t* off, uint8_t* bytes, jg_guid* guid, uint8_t* status);
/* keySpaces[key] (GetKeySpace, KeySpaceManager.cs:99-110): found[i], guid[i] (zero when absent). */
int jg_keyspace_lookup(jg_keyspace* ks, uint64_t n, const uint64_t* off, const uint8_t* key_bytes, jg_guid* guid, uint8_t* found);

/* ---------------------------------------------------------------------------------------------
 * Client reads by key name (csrc/query.hip) — additive to ABI v10.
 * PNCounterCommand / ORSetCommand "gp" / "gs" for a batch (CRDTCommands/PNCounterCommand.cs:27-41,
 * ORSetCommand.cs:28-42): KeySpaceManager.GetKVPair (KeySpaceManager.cs:138-142) ->
 * SafeCRDT.QueryStable / QueryProspective (SafeCRDT.cs:64-78) -> PNCounterWrapper.Query = PNCounter.Get
 * (PNCounters.cs:87-90) or ORSetWrapper.Query = ORSet.Contains(args[0]) (ORSetWrapper.cs:24-28).
 * One call chains the three resident tables on the device: the key space's dictionary (key -> Guid), the node's uid
 * table (Guid -> type, row | set id; pending jg_node_register entries are uploaded first) and, for an OR-Set read,
 * the store's element table (set, string -> element id); then jg_pnc_values' and jg_orset_contains' kernels answer.
 *
 * Query i reads key key_bytes[key_off[i], key_off[i+1]) (off[0] = 0 as elsewhere) on `node`, which is either copy of
 * the keyspace: the stable copy answers "gs", the prospective copy "gp" (a mixed batch is two calls).  elem_flag[i]:
 * 0 = no argument, 1 = the string elem_bytes[elem_off[i], elem_off[i+1]), 2 = the C# null element.  The three elem_*
 * pointers are all NULL (no query carries an argument) or all given.
 * Outputs: value[i] (Get's value, or Contains' 0 / 1; 0 for a status other than JG_Q_OK), status[i], kind[i] (optional: 0 PNCounter,
 * 1 ORSet, 255 unresolved), guid[i] (optional: keySpaces[key], zero when the dictionary lacks the key).
 *   Type.      The key's CRDT decides what is read, not the command (SafeCRDTManager hands back whichever SafeCRDT
 *              the key names): a PN-Counter key ignores any argument (PNCounterWrapper.Query never reads args).
 *   Argument.  An OR-Set key with flag 0 is JG_Q_NO_ARG (ORSetWrapper.Query dereferences args[0]); with flag 1 or 2
 *              the answer is Contains by string exactly as jg_orset_contains_names gives it: "", a name never seen,
 *              a set id without records and a name dropped by Clear are all absent.
 *   Overflow.  value and the overflow rule are jg_pnc_values' for the key's row: JG_Q_OVERFLOW with value 0 when a
 *              prefix of either checked Sum leaves the element type's range.
 *   Keys.      Compared byte for byte with the dictionary; a key holding a NUL byte is never in it (JG_Q_NO_KEY).
 *   JG_Q_NO_CRDT: the dictionary holds the key but `node` has nothing registered under its Guid (the reference's
 *              "Key not found" answer).
 * DEPARTURE (stated, parity-unpinned): the reference resolves safeCRDTs by key STRING (SafeCRDTManager.cs:29,72);
 * here keySpaces[key] gives a Guid and the node's uid table is asked for it.  The two differ only after a second local
 * CreateNewKVPair of a key the dictionary already holds: the reference rebinds safeCRDTs[key] to the new Guid's CRDT
 * while TryAdd (KeySpaceManager.cs:130) keeps the old Guid in keySpaces; this call keeps reading the old Guid's CRDT.
 * JG_EINVAL with every output untouched: NULL node, ks, value or status with n > 0; offsets that decrease (or
 * off[0] != 0); an elem_flag other than 0, 1, 2; only some of the elem_* pointers; a key space and a node of different
 * contexts.  n == 0 returns JG_OK.  The call holds the context's lock like jg_pnc_values and
 * jg_orset_contains_names, is not refused while a wave holds the stores (it then reads what the wave has applied so
 * far) unless a streamed wave of `node` itself is open with registrations pending, and changes no store or table. */
#define JG_Q_OK        0  /* value[i] valid */
#define JG_Q_NO_KEY    1  /* keySpaces[key] throws KeyNotFoundException (:140)                          */
#define JG_Q_NO_CRDT   2  /* the dictionary holds the key, the node has no CRDT under its guid: "Key not found" */
#define JG_Q_OVERFLOW  3  /* Get's checked Sum throws OverflowException                                  */
#define JG_Q_NO_ARG    4  /* an OR-Set key read without an element: ORSetWrapper.Query dereferences args */
int jg_node_query_keys(jg_node* node, jg_keyspace* ks, uint64_t n,
                       const uint64_t* key_off, const uint8_t* key_bytes,
                       const uint64_t* elem_off, const uint8_t* elem_bytes, const uint8_t* elem_flag,
                       int64_t* value, uint8_t* status, uint8_t* kind, jg_guid* guid);

/* ---------------------------------------------------------------------------------------------
 * Client writes by key name (csrc/update.hip) — additive to ABI v10.
 * PNCounterCommand "i" / "d" and ORSetCommand "a" / "r" / "c" for a batch (CRDTCommands/PNCounterCommand.cs:42-53,
 * ORSetCommand.cs:43-61): KeySpaceManager.GetKVPair -> SafeCRDT.Update(operationID, args) (SafeCRDT.cs:39-47) ->
 * prospectiveState.Update(operationID, args) in PNCounterWrapper (PNCounterWrapper.cs:33-48) or ORSetWrapper
 * (ORSetWrapper.cs:30-47).  One call resolves every key on the device through the key space's dictionary and the node's
 * uid table (as jg_node_query_keys; pending jg_node_register entries are uploaded first) and applies what resolved.
 *
 * Command i names key key_bytes[key_off[i], key_off[i+1]) (off[0] = 0 as elsewhere) on `node`, usually the prospective
 * copy's node (either copy is accepted).  op[i] is SafeCRDT.Update's operationID; arg_flag[i]: 0 = no argument, 1 = the
 * string elem_bytes[elem_off[i], elem_off[i+1]), 2 = the C# null, 3 = the integer amount[i].  tag_lo / tag_hi [i] is the
 * Guid.NewGuid() of an ORSet.Add (read for OR-Set commands only); col is the copy's own replica column
 * (PNCounters.cs:73-81).  Commands take effect in batch order.
 *   Type.      The key's CRDT decides what runs, not the command, as for reads.
 *   PN-Counter key.  PNCounterWrapper.Update evaluates (int)args[0] before its switch: an arg_flag other than 3 is
 *              JG_U_BAD_ARG (flag 0 or 2: NullReferenceException, flag 1: InvalidCastException).  With an integer, op 1
 *              is Increment(amount): the row's P cell at column col += amount; op 2 is Decrement(amount), the same on
 *              the N cell; both wrap at the store's width as jg_pnc_apply_ops does.  Any other op with an integer is
 *              JG_U_BAD_OP.  result[i] = 1 for an applied command.
 *   OR-Set key.  ORSetWrapper.Update switches first: an op outside 1..3 is JG_U_BAD_OP whatever the argument; op 3 is
 *              Clear and ignores the argument; op 1 is Add, op 2 Remove, both of the string (flag 1) or the null element
 *              (flag 2); flag 0 or 3 is JG_U_BAD_ARG.  Effects, result, elem, add_lim and rem_lim are exactly
 *              jg_orset_apply_ops_names' for the applied OR-Set commands, in batch order: its id rule, its Clear epochs,
 *              its ord limits.
 *   JG_U_NO_KEY / JG_U_NO_CRDT: as JG_Q_NO_KEY / JG_Q_NO_CRDT (a key of a kind whose store the node lacks is NO_CRDT).
 *   A failed command applies nothing and disturbs no other command (the reference catches per command): result 0,
 *              idx 0xFFFFFFFF, elem JG_NULL_ELEM - 1; kind is 0, 1 or 255 as for jg_node_query_keys.
 * Outputs: status[i], result[i]; optional: kind[i], idx[i] (the row or set the command touched: what a producer needs
 * to encode the snapshot SafeCRDT.Update ships next), elem[i] (the id an OR-Set command addressed, JG_NULL_ELEM - 1 for
 * every other command), guid[i] (keySpaces[key]), add_lim / rem_lim (both or neither; 0 for a command that is not an
 * applied OR-Set command).
 * DEPARTURE: keys are resolved by Guid, not by key string: the departure stated at jg_node_query_keys.
 * JG_EINVAL, decided from the arguments before anything is copied or written, every output and both stores untouched:
 * NULL node, ks, op, arg_flag, status or result with n > 0; offsets that decrease (or off[0] != 0); an arg_flag above 3;
 * an arg_flag 3 with amount NULL; an arg_flag 1 with elem_off or elem_bytes NULL; an arg_flag 1 or 2 with tag_lo or
 * tag_hi NULL (a PN-Counter-only batch may leave tags and elements NULL); col not below the PN-Counter store's replica
 * count (when the node has one); only one of add_lim / rem_lim; a key space and a node of different contexts; n >=
 * 2^31 - 16; a store held by an open wave; a streamed wave of `node` open with registrations pending.  n == 0 returns
 * JG_OK.
 * All or nothing: the resolve only reads; the OR-Set side, which can still refuse as jg_orset_apply_ops_names does (a set
 * out of element ids, an allocation), runs before any PN-Counter cell is written, and the PN-Counter adds cannot refuse
 * once launched: a refusal leaves both stores, the element table, the names log and every output as they were. */
#define JG_U_OK        0  /* applied (an OR-Set command's result[i] says whether it changed the set)            */
#define JG_U_NO_KEY    1  /* keySpaces[key] throws KeyNotFoundException                                          */
#define JG_U_NO_CRDT   2  /* the dictionary holds the key, the node has no CRDT under its guid                   */
#define JG_U_BAD_ARG   3  /* args[0] absent, null or of the wrong type for the key's CRDT                        */
#define JG_U_BAD_OP    4  /* the wrapper's switch has no case for the operation id                               */
int jg_node_update_keys(jg_node* node, jg_keyspace* ks, uint64_t n,
                        const uint64_t* key_off, const uint8_t* key_bytes,
                        const uint8_t* op, const uint8_t* arg_flag, const int64_t* amount,
                        const uint64_t* elem_off, const uint8_t* elem_bytes,
                        const uint64_t* tag_lo, const uint64_t* tag_hi, uint32_t col,
                        uint8_t* status, uint8_t* result, uint8_t* kind, uint32_t* idx, uint32_t* elem,
                        jg_guid* guid, uint64_t* add_lim, uint64_t* rem_lim);

/* ---------------------------------------------------------------------------------------------
 * Client writes by key name that also ship their PN-Counter snapshots (csrc/update.hip, csrc/pnc_encode.hip) —
 * additive to ABI v10.
 * Both halves of SafeCRDT.Update (SafeCRDT.cs:39-62) for a batch: prospectiveState.Update(operationID, args), which is
 * jg_node_update_keys, and syncMsg.message = prospectiveState.crdt.GetLastSynchronizedUpdate().Encode(), the bytes
 * the client batcher hashes and submits.  Every argument jg_node_update_keys takes means here what it means there:
 * the same statuses, refusals, outputs and all-or-nothing rule.  Added: snap (one byte per command; NULL = 1 for every
 * command), snap_off (n + 1 entries, snap_off[0] = 0, always filled), out / cap (the snapshots' bytes and the room
 * for them), sha (NULL, or n x 32 bytes).
 *   Snapshot.  Command i's snapshot is out[snap_off[i], snap_off[i+1]): GetLastSynchronizedUpdate().Encode()
 *              (PNCounters.cs:115-118, 46-49) of the key's row right after command i, i.e. the row before the call plus
 *              every applied PN-Counter command j <= i of the batch on the same row (whatever snap[j] says), wrapping at
 *              the store's width.  The bytes are exactly jg_pnc_apply_ops_encode's for the same ops on the same row;
 *              sha + 32 i is their SHA-256 (ComputeDigest's first level) when sha is given.
 *   Who gets one.  Command i, iff it is an applied PN-Counter command (status JG_U_OK, kind 0) and
 *              snap[i] == 1: a safe update, which the batcher ships individually (SafeCRDTManager.cs:178-181); or
 *              snap[i] == 2 and no later command j > i of the call with snap[j] == 2 is an applied PN-Counter command on
 *                            the same row: the batcher's compaction, appearedObjects[np.uid] = np (:179, 186-187), which
 *                            keeps only the latest non-safe state of an object.  The survivors are decided on the device
 *                            from the resolved rows (the host never learns which key strings name one object).  A call
 *                            is ONE batcher batch for this rule: a caller whose batcher flushes mid-batch makes one call
 *                            per flush.
 *              snap[i] == 0: none.  Every command without a snapshot (snap 0, a 2 that did not survive, any failed
 *              status, every OR-Set command) has snap_off[i+1] == snap_off[i] and 32 zero bytes of sha.
 *   OR-Set commands are applied exactly as jg_node_update_keys applies them and get no bytes from this call (add_lim /
 *              rem_lim say where jg_orset_encode_json would cut).  The LIMIT this was is lifted by
 *              jg_node_update_keys_ship below, which ships every kind's snapshots from one call.
 * JG_EINVAL in addition to jg_node_update_keys' list, every output and both stores untouched: snap_off NULL; a snap[i]
 * above 2; out NULL while the batch could ship a snapshot, which is decided from the arguments alone: a command with
 * arg_flag 3 whose snap is not 0 (or snap NULL).
 * JG_ESTATE: snap_off[n] > cap.  snap_off is filled and NOTHING is applied (the OR-Set commands, the element table and
 * the names log included; every other output untouched): the PN-Counter length pass and this check run before the
 * OR-Set side writes anything, and the OR-Set side, which can still refuse, runs before any PN-Counter cell is written.
 * The caller calls again with a larger out.
 * A node without a PN-Counter store, and a batch whose commands all fail, succeed with every snap_off entry 0.
 * n == 0 returns JG_OK with snap_off[0] = 0. */
int jg_node_update_keys_encode(jg_node* node, jg_keyspace* ks, uint64_t n,
                               const uint64_t* key_off, const uint8_t* key_bytes,
                               const uint8_t* op, const uint8_t* arg_flag, const int64_t* amount,
                               const uint64_t* elem_off, const uint8_t* elem_bytes,
                               const uint64_t* tag_lo, const uint64_t* tag_hi, uint32_t col, const uint8_t* snap,
                               uint8_t* status, uint8_t* result, uint8_t* kind, uint32_t* idx, uint32_t* elem,
                               jg_guid* guid, uint64_t* add_lim, uint64_t* rem_lim,
                               uint64_t* snap_off, uint8_t* out, uint64_t cap, uint8_t* sha);

/* ---------------------------------------------------------------------------------------------
 * Client writes by key name that ship every snapshot, OR-Set keys included (csrc/update.hip, csrc/pnc_encode.hip,
 * csrc/orset_encode.hip) — additive to ABI v10.
 * SafeCRDT.Update (SafeCRDT.cs:39-62) for a whole batcher batch of any mix of keys: one call applies every command and
 * returns, per command, the bytes of prospectiveState.crdt.GetLastSynchronizedUpdate().Encode() the batcher ships.
 * Every argument shared with jg_node_update_keys_encode means what it means there: the statuses, the type rule, JG_U_*,
 * kind / idx / elem / guid, snap (NULL = 1 for every command), snap_off (n + 1 entries, snap_off[0] = 0), sha (NULL or
 * n x 32 bytes, 32 zero bytes for a command that ships nothing).  There is no add_lim / rem_lim: the snapshots replace
 * them, and across rounds they would mean nothing.
 *   PN-Counter commands.  Exactly as in jg_node_update_keys_encode: the same survivors, bytes and hashes.
 *   OR-Set commands.  Applied exactly as jg_node_update_keys applies them (jg_orset_apply_ops_names' id rule, Clear
 *              epochs, result and elem).  Command i's snapshot is ORSetMsg.Encode() (ORSet.cs:56-69, 305-308) of its set
 *              as it stood right after command i: byte for byte jg_orset_encode_json's state of that set at command i's
 *              ord limits, taken before any later Clear of the set is applied.
 *   Who gets one.  Command i, iff it is an applied OR-Set command (status JG_U_OK, kind 1) and snap[i] == 1, or
 *              snap[i] == 2 and no later applied OR-Set command with snap == 2 is on the same set (the batcher's
 *              appearedObjects[np.uid] = np, SafeCRDTManager.cs:179, 186-187).  The op and its result do not matter: a
 *              Remove that returned 0 and a Clear both ship (SafeCRDT.Update encodes whatever Update returned).  Both
 *              kinds' survivors are decided on the device from the resolved object ids.
 *   Rounds.    A Clear drops records a snapshot taken before it still needs, so the library applies the OR-Set commands
 *              in rounds: per set, in batch order, a Clear starts a new round iff a shipping command on that set lies
 *              between the set's previous Clear (or the batch start) and it; a command's round is the number of such
 *              Clears of its own set at or before it.  Round r's commands are applied in batch order, then the round's
 *              shipping commands are encoded.  *n_rounds (optional) is the number of rounds run: 0 for a batch without an
 *              applied OR-Set command.  The stores end as after jg_orset_apply_ops_names over each round in turn.
 *   The image. out[snap_off[i], snap_off[i+1]) is command i's snapshot, whatever its kind, in command order.  The image is
 *              merged on the device and crosses the host link once.
 *   Size.      The lengths of OR-Set snapshots are known only after their round is applied, so this call never refuses
 *              for cap: *n_bytes (required) always receives snap_off[n]; if *n_bytes <= cap the bytes are copied to out,
 *              else out is untouched, the call still returns JG_OK with everything applied, snap_off and sha filled,
 *              and the node HOLDS the image on the device for jg_node_shipped.  out NULL with cap 0 means "hold it".
 * jg_node_shipped(node, &nb, out, cap) fetches the held image: out NULL = size query; JG_ESTATE if cap is short (the image
 * stays held); a successful fetch releases it; with nothing held JG_OK with *n_bytes = 0.  The held image is dropped by
 * the next jg_node_update_keys_ship on the node that ships a byte and by jg_node_destroy.
 * Refusals, all before anything is written (every output, both stores, the element table and the names log untouched):
 * jg_node_update_keys' JG_EINVAL list; a snap[i] above 2; snap_off or n_bytes NULL; out NULL with cap > 0.
 * JG_ESTATE: a set that would ship holds a record whose element id has no name in the store's table (records put
 * there by jg_orset_load without jg_orset_names_sync) — the same set in a batch that ships nothing from it is applied
 * as ever; or the batch has more than one round and the fullest set's next element id plus the most Adds the batch
 * has on one set could pass the id limit (conservative; with one round jg_orset_apply_ops_names' own check decides).
 * Round 0's apply can still refuse as jg_orset_apply_ops_names does, and then nothing has been written.
 * ONCE ROUND 0 HAS WRITTEN, only an allocation failure or a HIP error can stop a later round (jg_apply_committed's rule
 * for its OR-Set commit): the code is returned, the PN-Counter store is untouched (its adds run last) and the OR-Set
 * store must be reloaded.
 * n == 0 returns JG_OK with snap_off[0] = 0, *n_bytes = 0 and *n_rounds = 0. */
int jg_node_update_keys_ship(jg_node* node, jg_keyspace* ks, uint64_t n,
                             const uint64_t* key_off, const uint8_t* key_bytes,
                             const uint8_t* op, const uint8_t* arg_flag, const int64_t* amount,
                             const uint64_t* elem_off, const uint8_t* elem_bytes,
                             const uint64_t* tag_lo, const uint64_t* tag_hi, uint32_t col, const uint8_t* snap,
                             uint8_t* status, uint8_t* result, uint8_t* kind, uint32_t* idx, uint32_t* elem, jg_guid* guid,
                             uint64_t* snap_off, uint64_t* n_bytes, uint8_t* out, uint64_t cap, uint8_t* sha,
                             uint32_t* n_rounds);
int jg_node_shipped(jg_node* node, uint64_t* n_bytes, uint8_t* out, uint64_t cap);

/* ---------------------------------------------------------------------------------------------
 * Client batches by key name: reads in order among the writes (csrc/update.hip, csrc/pnc.hip) — additive to ABI v10.
 * A connection's stream of commands as the reference's workloads send it: PNCWorkload draws "i" / "d" / "gp" over its
 * keys round-robin (BenchmarkClient PNCWorkload.cs:44-59), ORSetWorkload "a" / "gp" on one key until its Clear
 * (ORSetWorkload.cs:66-138), half of them reads, and the server runs each command to completion before the next
 * (PNCounterCommand.cs:27-53, ORSetCommand.cs:28-69, under lock (instance)): a "gp" sees exactly the writes before it.
 * The call behaves as if the commands ran one at a time, in batch order, on `node`: a write (cmd[i] == 0,
 * SafeCRDT.Update, SafeCRDT.cs:39-62) as a one-command jg_node_update_keys_ship, a read (cmd[i] == 1,
 * SafeCRDT.QueryProspective, SafeCRDT.cs:64-78) as a one-command jg_node_query_keys, with one exception: the survivors
 * of snap == 2 are decided over the whole call as jg_node_update_keys_ship decides them (one call is one batcher batch).
 * `node` is usually the prospective copy (either copy is accepted, and a read answers from whichever copy it is);
 * "gs" reads do not depend on the batch and stay with jg_node_query_keys on the stable node.
 *   Writes.    Every argument, status (JG_U_*), output, snapshot, hash, round, refusal and all-or-nothing rule is
 *              jg_node_update_keys_ship's.  Reads are invisible to writes: deleting the reads from a batch leaves the same
 *              stores, element table and names log, the same status / result / kind / idx / elem / guid for the writes,
 *              the same image bytes in the same order, the same sha and the same *n_rounds.  value[i] of a write is 0.
 *   Reads.     status[i] is a JG_Q_* code under jg_node_query_keys' rules: the key's CRDT decides, a PN-Counter key
 *              ignores any argument, an OR-Set key with arg_flag 0 is JG_Q_NO_ARG (with 1 or 2 it reads the string or the
 *              null element); JG_Q_NO_KEY / JG_Q_NO_CRDT as there.  kind, idx (the row or set read) and guid as for
 *              writes; elem is the id the read addressed, JG_NULL_ELEM - 1 where no record carries one; result[i] = 0.
 *              A read never ships (snap_off[i+1] == snap_off[i], 32 zero bytes of sha), never opens or cuts a round,
 *              and never counts as a later command for the snap == 2 rule of either kind.  snap[i], op[i], tag_*[i] and
 *              amount[i] of a read are ignored.
 *   PN-Counter read.  value[i] is PNCounter.Get (PNCounters.cs:87-90) of the row as it stood before the call plus every
 *              applied PN-Counter write j < i of this call on the same row: op 1 amounts added to the P cell at column
 *              col, op 2 amounts to the N cell, each wrapping at the store's width, then jg_pnc_values' checked sums in
 *              column order: JG_Q_OVERFLOW with value 0 when a prefix of either sum leaves the range.  An overflow may
 *              appear or disappear because of an earlier write of the batch; the write is applied either way.
 *   OR-Set read.  value[i] is ORSet.Contains(args[0]) (ORSetWrapper.cs:24-28, ORSet.cs:204-237) on the set after every
 *              applied OR-Set write j < i of this call on the same set.  The name resolves as a Remove's does
 *              (jg_orset_apply_ops_names): a name first Added earlier in the batch has the id that Add was issued, a
 *              name the set never held, or dropped by a Clear and not re-added, is absent; a read interns nothing.
 *              Membership is Remove's own test over the element's tags at that point.  A batch whose OR-Set commands
 *              are all reads writes neither the store, the element table nor the names log.
 * JG_EINVAL, decided from the arguments with everything untouched: jg_node_update_keys_ship's list with cmd and value
 * added to the required pointers; a cmd[i] above 1; a read with arg_flag 3.  tag_lo / tag_hi are required only when a
 * WRITE carries an element, amount only when a write carries an integer, op only when the batch has a write: a batch
 * of reads only is legal with op, amount, the tags and snap NULL.  Like jg_node_update_keys_ship, and unlike
 * jg_node_query_keys, the call is refused while a wave holds a store.
 * An image larger than cap is held on the node and fetched with jg_node_shipped.  n == 0 as jg_node_update_keys_ship. */
int jg_node_exec_keys(jg_node* node, jg_keyspace* ks, uint64_t n,
                      const uint64_t* key_off, const uint8_t* key_bytes,
                      const uint8_t* cmd,
                      const uint8_t* op, const uint8_t* arg_flag, const int64_t* amount,
                      const uint64_t* elem_off, const uint8_t* elem_bytes,
                      const uint64_t* tag_lo, const uint64_t* tag_hi, uint32_t col, const uint8_t* snap,
                      uint8_t* status, uint8_t* result, int64_t* value, uint8_t* kind, uint32_t* idx, uint32_t* elem,
                      jg_guid* guid,
                      uint64_t* snap_off, uint64_t* n_bytes, uint8_t* out, uint64_t cap, uint8_t* sha,
                      uint32_t* n_rounds);

/* ---------------------------------------------------------------------------------------------
 * CRDT creation on the device (csrc/adopt.hip) — additive to ABI v10.
 * The reference creates a CRDT on its receive path: ReplicationManager.ReceivedNewObjectSyncMsg
 * (ReplicationManager.cs:310-324) records uid -> type when a ManagerMsg_Create arrives (CreateCRDTInstance), and
 * KeySpaceManager.OnNext (KeySpaceManager.cs:151-178) calls SafeCRDTManager.CreateSafeCRDT(key, guid)
 * (SafeCRDTManager.cs:86-101) for every key it learns, which reads the type back with rm.GetCRDTType(guid) and creates
 * the stable instance.  Here the node allocates the rows: the caller keeps neither a row allocator nor a
 * uid -> (type, row) map, and a learnt key becomes a usable CRDT without leaving the device.
 *
 * ALLOCATION (per node, per kind).  The next PN-Counter row is one past the largest row registered on the node by any
 * path (jg_node_register included), 0 with none; the next set id likewise.  Within one call the created entries of a
 * kind take consecutive indices in call order.  jg_node_next_idx reads both (either pointer may be NULL).
 * When the rows a call needs pass the store's n_keys the store grows as jg_pnc_reserve grows it, to
 * max(needed, 2 x n_keys) clipped to max_keys; JG_ESTATE when needed > max_keys (max_keys 0: the store never grows),
 * when the set ids would pass 2^31 - 16, or when `replica` has no free column in a row someone interned by hand.
 * jg_pnc_reserve's own refusals (an open jg_pnc_wave_begin wave: JG_EINVAL; allocation: JG_ENOMEM) pass through.
 * ALL OR NOTHING: a call that returns a code other than JG_OK has changed no table, no store and no output.
 *
 * jg_node_create_uids — a batch of ReceivedNewObjectSyncMsg / CreateCRDTInstance, in call order.  type[i]: 0 PNCounter,
 * 1 ORSet (the caller maps NetworkProtocol.type strings; an unregistered type string is its ArgumentException).
 * replica: NULL, or one Guid per entry: a created PN-Counter's replica[i] is interned in the new row as jg_pnc_intern
 * would intern it (the PNCounter() constructor's {self: 0}, PNCounters.cs:73-81; column 0 of a fresh row); ignored for
 * ORSet entries; with NULL no column is interned.  status[i]: JG_C_CREATED, or JG_C_EXISTS when the uid is on the node
 * already, however it got there, or is repeated earlier in the batch (the first occurrence in call order wins): then
 * no row is consumed and nothing is interned.  idx[i] (optional) = the entry's row / set id, the existing one for
 * JG_C_EXISTS (which may be of the other kind than type[i]).
 * DEPARTURE (stated): the reference's objectLookupTable[uid] = crdtObject (ReplicationManager.cs:320) replaces the
 * object of an uid created twice with an empty one; here the first creation stands.
 * JG_EINVAL, decided before anything is written: NULL node, uid, type or status with n > 0; Guid.Empty; a type above 1;
 * a kind whose store the node lacks; n >= 2^31 - 16; a streamed wave of the node open, or a wave holding a store.
 * A created uid of another shard turns the shard shortcut off as jg_node_register does.  n == 0 returns JG_OK.
 *
 * jg_node_adopt_keys — OnNext's CreateSafeCRDT(key, guid) for journal records [from, to) of `ks` (the journal
 * jg_keyspace_new_keys reads; to <= its length), in journal order, on the `stable` copy; the records never leave the
 * device.  Outputs at j - from.  status:
 *   JG_A_SKIPPED   the record's journal status is 1, 2 or 3 (no key was added);
 *   JG_A_NO_TYPE   `prospective` holds no CRDT under the record's Guid: GetCRDTType throws KeyNotFoundException
 *                  (ReplicationManager.cs:329).  The dictionary holds the key already, so reads and writes by that name
 *                  answer NO_CRDT, as in the reference, until the uid is created and the range adopted again;
 *   JG_A_HAVE      `stable` holds the Guid, or an earlier record of the range names it (two keys bound to one Guid:
 *                  the departure stated at jg_node_query_keys): kind / idx of that entry;
 *   JG_A_ADOPTED   the kind is read from `prospective`, a row or set id is allocated on `stable` and the uid
 *                  registered; a PN-Counter's replica[j - from] is interned in the new row when replica is not NULL.
 * kind (0 PNCounter, 1 ORSet) and idx are optional; a record that is neither adopted nor held gets 255 / 0xFFFFFFFF.
 * `prospective` is only read (its pending registrations are uploaded first, as for the by-name calls).  The call may
 * be repeated over a range: records that are JG_A_HAVE by then change nothing.
 * JG_EINVAL as for jg_node_create_uids, and: NULL stable, prospective, ks or status; from > to or to past the journal;
 * handles of different contexts; a kind `stable` has no store for. */
#define JG_C_CREATED 0
#define JG_C_EXISTS  1
#define JG_A_ADOPTED 0
#define JG_A_HAVE    1
#define JG_A_NO_TYPE 2
#define JG_A_SKIPPED 3
int jg_node_next_idx(jg_node* node, uint32_t* next_row, uint32_t* next_set);
int jg_node_create_uids(jg_node* node, uint64_t n, const jg_guid* uid, const uint8_t* type,
                        const jg_guid* replica, uint64_t max_keys, uint8_t* status, uint32_t* idx);
int jg_node_adopt_keys(jg_node* stable, jg_node* prospective, jg_keyspace* ks, uint64_t from, uint64_t to,
                       const jg_guid* replica, uint64_t max_keys, uint8_t* status, uint8_t* kind, uint32_t* idx);

/* ---------------------------------------------------------------------------------------------
 * Synthetic workloads (bench / size-independent parity): device-side counter-based generators,
 * defined in DESIGN.md §Synthetic inputs and mirrored on the host by the test oracle.
 * ------------------------------------------------------------------------------------------- */
/* which: 0 = local P, 1 = local N, 2 = received P, 3 = received N.  Local unseen cells are 0;
 * received unseen cells are ABSENT.  jg_synth_pnc_rows fills the values of row i from synthetic key
 * key0 + i and keeps the batch's key indices (identity unless uploaded). */
int jg_synth_pnc_store(jg_pnc* pnc, uint64_t seed);
int jg_synth_pnc_rows(jg_rows* rows, uint64_t seed, uint64_t key0);
/* Fill a store with n_groups (set, elem) groups (group g = set*elems_per_set + elem): adds carry
 * tags u in [add_u0, add_u0+add_per_group), tombstones u in [rem_u0, rem_u0+rem_per_group). */
int jg_synth_orset(jg_orset* s, uint64_t seed, uint64_t n_groups, uint32_t elems_per_set,
                   uint32_t add_per_group, uint32_t add_u0, uint32_t rem_per_group, uint32_t rem_u0);

#ifdef __cplusplus
}
#endif

#endif /* JANUS_GPU_H */
