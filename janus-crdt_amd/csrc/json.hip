// json.hip — committed state messages applied straight from their wire bytes (SURVEY.md §8f F1 + A2/A13).
//
// The reference's stable apply decodes every committed state with System.Text.Json and merges it:
// SafeCRDT.ApplyUpdateStable (BFT-CRDT/SafeCRDTs/SafeCRDT.cs:80-83) -> PNCounter.DecodePropagationMessage
// -> PNCounterMsg.Decode (MergeSharp/MergeSharp/CRDTs/PNCounters.cs:38-43) -> Merge (:131-144), one
// message at a time inside HandleAfterConsensusUpdates (SafeCRDTManager.cs:109-160).  Here a whole
// wave of PNCounterMsg JSON payloads is uploaded once and decoded, interned and merged on the GPU:
//
//   pass A  k_scan      8 lanes per message (json_wave.hpp) prove the payload is the compact form
//                       System.Text.Json writes and check it against the wire contract of
//                       oracle/json.hpp; every Guid is looked up in its row's replica table (read-only);
//                       a Guid repeated among a vector's known replicas sends the message to the serial
//                       parser (System.Text.Json keeps the key's last value at its first place).  Each message
//                       leaves a record: its entries' columns and values (pass B applies it), or, when
//                       it names a replica its row has not seen (DEFERRED, marked per message), the
//                       entries' Guids and values with the columns still open.  Payloads not in the
//                       compact form go to the slow list: k_scan_slow runs the serial parser on them.
//   host     deferral marks compacted (hipcub select, count written beside the status) and one
//            D2H of the status words: first bad message, deferred count.  A bad message = nothing
//            is written.
//   sort     hipcub radix sort of the deferred list -> messages grouped by row in commit order.
//   pass C   k_resolve_rows  one lane per row segment walks the row's deferred records in commit
//                       order and appends the new replica Guids (pVector entries first, then nVector —
//                       Merge's order) to the row's table: first-insertion order = the stable
//                       Dictionary's enumeration order; the columns go back into the records.  A walk
//                       reaching a non-compact message continues serially (k_resolve_resume).  A Guid
//                       repeated in one vector keeps its first place and its last value (the earlier
//                       entries are voided).  A full row rolls the appended columns back and fails the call.
//   pass B  k_apply_emit  one lane per record entry, atomicMax into P / N (messages of one wave may
//                       repeat a key; max is order-free); k_apply_list parses the slow list again.
//
// Fused pass A (round 5, the default; JANUS_JSON_FUSE=0 turns it off): a message whose replicas are all known
// is applied by pass A itself once its checks are done, and its record then holds only the entries that
// raised their cell, each with the cell's old value.  All or nothing still holds: max has no inverse, but a
// cell's smallest recorded old value is its value before the wave whatever order the raises took, so a wave
// that fails later (a bad message, a full row, a node wave cut or aborted) is undone exactly by atomicMin over
// the records (k_undo_applied).  The steady state — every replica known, the common wave — writes no record
// entries at all when its states repeat the cells and runs no pass B: the 64-byte records pass B read back and
// the second touch of every cell's lines (pass A + pass B moved 3.1x the algorithmic bytes) go.
//
// JANUS_JSON_GROUP=1 runs the serial parser (scan_one / resolve_one / apply_one: byte-serial per thread
// through a 16-byte window register) for every message: the reference the group path is tested
// against.  The bound of the end-to-end call is the PCIe upload of the payload.
//
// The PN-Counter wire path's files:
//   pnc_wire.hpp         the wire form: Guid16, Table, the serial parser and passes, pass A's record format
//   json_wave.hpp        the group kernels of passes A, B and C (this file's only)
//   pnc_table.hpp        the replica table's allocation and the row-key sort (shared with pnc_encode.hip)
//   pnc_wave_layout.hpp  the wave's status block: status words, deferred list, roll-back slots (no HIP type)
//   json.hip             a wave decoded and merged, its entry points; the only writer of jg::PncWave
//   pnc_encode.hip       the other direction: rows encoded as PNCounterMsg JSON, the producer's apply-ops calls
#include <cstring>

#include "json_wave.hpp"
#include "pnc_table.hpp"
#include "pnc_wave_layout.hpp"

namespace {

// Chunk offsets arrive relative to their chunk: add the chunk's byte base.
__global__ void k_rebase(uint64_t* __restrict__ off, uint64_t n, uint64_t base) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) off[i] += base;
}

// The row's count back to its value before the walk, and every slot past it zeroed: a failed walk may have
// written columns it never counted (k_resolve_rows keeps its count in a register until the row is done),
// and pass A reads a row's columns as its leading non-zero slots (json_wave.hpp row_cache).
__global__ __launch_bounds__(kBlock) void k_rollback(const unsigned long long* __restrict__ keys, uint64_t nd, Table t,
                                                     const uint32_t* __restrict__ saved) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= nd) return;
    const uint32_t row = (uint32_t)(keys[i] >> 32);
    if (i > 0 && (uint32_t)(keys[i - 1] >> 32) == row) return;
    t.ncols[row] = saved[i];
    for (uint32_t c = saved[i]; c < t.R; ++c) t.cols[(uint64_t)row * t.R + c] = Guid16{0, 0};
}

// jg_pnc_intern: entries (row, guid) in order; keys = row << 32 | i sorted; segment heads walk.
__global__ __launch_bounds__(kBlock) void k_intern(const unsigned long long* __restrict__ keys, uint64_t n, const Guid16* __restrict__ g,
                                                   Table t, uint32_t* __restrict__ col_out, uint32_t* __restrict__ saved,
                                                   unsigned long long* __restrict__ status) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t row = (uint32_t)(keys[i] >> 32);
    if (i > 0 && (uint32_t)(keys[i - 1] >> 32) == row) return;
    uint32_t* ncol = t.ncols + row;
    Guid16* cols = t.cols + (uint64_t)row * t.R;
    saved[i] = *ncol;
    for (uint64_t j = i; j < n && (uint32_t)(keys[j] >> 32) == row; ++j) {
        const uint32_t e = (uint32_t)keys[j];
        uint32_t c = find_col(cols, *ncol, g[e], UINT32_MAX);
        if (c == UINT32_MAX) {
            if (*ncol >= t.R) {
                atomicMin(status + 2, (unsigned long long)e << 2 | kErrFull);
                return;
            }
            c = (*ncol)++;
            cols[c] = g[e];
        }
        col_out[e] = c;
    }
}

__global__ void k_gather_cols(const Guid16* __restrict__ cols, const uint32_t* __restrict__ ncols, const uint32_t* __restrict__ rows,
                              uint64_t n, uint32_t R, Guid16* __restrict__ out, uint32_t* __restrict__ nout) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n * R) return;
    const uint64_t q = i / R, c = i - q * R;
    const uint32_t row = rows[q];
    out[i] = cols[(uint64_t)row * R + c];
    if (c == 0) nout[q] = ncols[row];
}

using jg::blocks_for;
using jg::grow_keep;

struct IsDeferred {
    __host__ __device__ bool operator()(const unsigned long long& k) const { return k != kNotDeferred; }
};

// Pass A's per-message deferral marks (n of them) compacted into a list, its length written to *count
// on the device; then sorted by (row, message) = commit order within each row.  Marks and a compaction
// instead of an appended list or a counter: every wave touching one address serialises the grid at
// that address's L2 channel — a cold wave (every message deferred) measured 1.5 ms for pass A instead
// of 0.33 with one non-returning atomic per wave.
struct DeferredLists {
    unsigned long long* list;    // n slots
    unsigned long long* sorted;  // n slots
    void* tmp;
    size_t tmp_bytes;
    int end_bit;
};

DeferredLists select_deferred(jg_ctx* ctx, const unsigned long long* marks, uint64_t n, uint64_t n_keys, unsigned long long* count) {
    using ull = unsigned long long;
    const int items = jg::cub_count(n, "wave entries");
    DeferredLists d{};
    d.end_bit = row_end_bit(n_keys);
    const auto select = [&](void* temp, size_t& bytes) {
        return hipcub::DeviceSelect::If(temp, bytes, marks, d.list, count, items, IsDeferred(), ctx->stream);
    };
    // the select and the sort that follows it (sort_deferred) share one workspace
    d.tmp_bytes = std::max(jg::cub_temp_bytes(select), jg::cub_temp_bytes([&](void* temp, size_t& bytes) {
                               return sort_row_keys(temp, bytes, (const ull*)nullptr, (ull*)nullptr, n, d.end_bit, ctx->stream);
                           }));
    uint8_t* tmp;
    jg::Layout L;
    L.add(d.list, n), L.add(d.sorted, n), L.add(tmp, d.tmp_bytes + 256);
    L.bind(jg::scratch(ctx, ctx->scratch3, L.bytes()));
    d.tmp = tmp;
    jg::cub_run(jg::cub_in(d.tmp, d.tmp_bytes), select);
    return d;
}

// The list comes out of the (stable) select in message order, so a stable sort on the row bits alone gives the
// order of the whole key (row, then message): 20 bits for 1M keys instead of 52.
unsigned long long* sort_deferred(jg_ctx* ctx, DeferredLists& d, uint64_t nd) {
    jg::cub_run(jg::cub_in(d.tmp, d.tmp_bytes),
                [&](void* temp, size_t& bytes) { return sort_row_keys(temp, bytes, d.list, d.sorted, nd, d.end_bit, ctx->stream); });
    return d.sorted;
}

struct Status { unsigned long long first_bad, n_deferred, resolve_bad, n_slow, n_resume; };

static_assert(sizeof(Status) <= 256, "status fits the context's page-locked word");

// Into the context's page-locked bytes: a pageable destination is staged by the runtime (a blit plus a host
// copy per read; three reads per wave)
Status read_status(jg_ctx* ctx, const unsigned long long* d) {
    Status s;
    jg::pin_get(ctx, 0, d, sizeof s);
    jg::pin_sync(ctx);
    std::memcpy(&s, jg::pin_at(ctx, 0), sizeof s);
    return s;
}

// kErrInternal (a message pass A accepted that a later pass could not parse or resolve again) is the library's
// own inconsistency, never a verdict on the message: it leaves *bad_msg unset, so a node wave does not take it for
// the reference's cut (pnc_node_finish rethrows, wave_end aborts the wave) and no caller blames the payload.
// kErrFull's error: the one failure the opt-in widening (jg_pnc_set_max_replicas) answers by running the call again
// on a wider store.  Everyone else catches it as the jg::Error it is (JG_ESTATE, the same text as ever).
struct RowFull : jg::Error {};

[[noreturn]] void fail_msg(unsigned long long code, uint64_t* bad_msg, const char* what) {
    const uint64_t m = code >> 2;
    const uint32_t kind = (uint32_t)(code & 3);
    if (bad_msg && kind != kErrInternal) *bad_msg = m;
    if (kind == kErrFull) {
        char msg[160];
        std::snprintf(msg, sizeof msg, "%s %llu: its key holds more replicas than the store's columns", what, (unsigned long long)m);
        throw RowFull{{JG_ESTATE, msg}};
    }
    if (kind == kErrInternal) jg::fail(JG_EHIP, "%s %llu: internal replica-table inconsistency", what, (unsigned long long)m);
    jg::fail(JG_EINVAL, "%s %llu is not a PNCounterMsg in the accepted JSON form (JsonException)", what, (unsigned long long)m);
}

// Wave-level device scratch: status words, pass A's deferred marks and the roll-back slots (n messages),
// pass A's per-message entries and its list of messages for pass B to parse again.
struct WaveScratch {
    unsigned long long* status;
    unsigned long long* deferred;
    uint32_t* saved;
    uint8_t* emit;
    Guid16* eguid;  // [n x kEmitMax] entry Guids of the deferred compact messages
    unsigned long long* slow;
};

// Room for n messages; growing keeps the status words and the first `keep` messages' deferred marks and
// records (a streamed wave grows between chunks).  The status block is pnc_wave_layout.hpp's.
WaveScratch wave_scratch(jg_pnc* p, uint64_t n, uint64_t keep = 0) {
    jg::PncWave& v = p->wave;
    grow_keep(p->ctx, v.stat, jg::wave_status_bytes(n), jg::wave_status_keep(keep));
    grow_keep(p->ctx, v.emit, n * emit_stride(p->eb) + 256, keep * emit_stride(p->eb));
    grow_keep(p->ctx, v.slow, n * 8 + 256, keep * 8);
    grow_keep(p->ctx, v.guid, n * kEmitMax * sizeof(Guid16) + 256, keep * kEmitMax * sizeof(Guid16));
    WaveScratch w{nullptr, nullptr, nullptr, v.emit.as<uint8_t>(), v.guid.as<Guid16>(), v.slow.as<unsigned long long>()};
    jg::carve_wave_status(jg::wave_status_capacity(v.stat.bytes), v.stat.p, w);  // the capacity actually there
    return w;
}

__global__ void k_reset_status(unsigned long long* status) {
    const unsigned long long init[5] = {~0ull, 0, ~0ull, 0, 0};  // Status{first_bad, n_deferred, resolve_bad, n_slow, n_resume}
    if (threadIdx.x < 5) status[threadIdx.x] = init[threadIdx.x];
}

// a one-wave kernel instead of a copy from pageable host memory (staged by the runtime: a blit and a host
// round trip in front of every wave's pass A)
void reset_status(jg_ctx* ctx, unsigned long long* status) {
    hipLaunchKernelGGL(k_reset_status, dim3(1), dim3(64), 0, ctx->stream, status);
    JG_HIP(hipGetLastError());
}

// A wave's status words at their initial values: reset on the device unless the last wave left them so (a
// clean wave — nothing bad, deferred, slow or resumed — never writes them: round 6 skips the reset launch).
void begin_status(jg_pnc* p, unsigned long long* status) {
    if (!p->wave.status_clean) reset_status(p->ctx, status);
    p->wave.status_clean = false;
}

// A wave of up to `cap` messages begins (merge_wave_dev, jg_pnc_wave_begin, pnc_node_begin): the table and the
// scratch are there, the status words are ready, nothing is scanned.  The one place JANUS_JSON_FUSE is read
// (=0: pass A leaves every message to pass B; tests and A/B runs switch it): the chunks' pass A and the wave's
// finish must agree on it, or finish_wave would skip pass B for records pass A left to it.
WaveScratch begin_wave(jg_pnc* p, uint64_t cap) {
    ensure_table(p);
    const WaveScratch w = wave_scratch(p, cap);
    begin_status(p, w.status);
    p->wave.scan_hi = 0;
    const char* e = std::getenv("JANUS_JSON_FUSE");
    p->wave.fuse = !(e && std::strcmp(e, "0") == 0);
    return w;
}

void launch_scan(jg_pnc* p, const uint8_t* bytes, const uint64_t* off, const uint32_t* rows, uint64_t m0, uint64_t m1,
                 const WaveScratch& w) {
    if (m1 <= m0) return;
    const Table t = table_of(p);
    const int G = json_group();
    const bool fuse = p->wave.fuse;
    jg::dispatch_eb(p->eb, [&](auto EB) {
        launch_scan_g<EB()>(G, p->ctx->stream, bytes, off, rows, m0, m1, t, w.status, w.deferred, w.emit, w.eguid, w.slow, p->rw_P(), p->rw_N(), fuse);
    });
    JG_HIP(hipGetLastError());
    p->wave.scan_hi = std::max(p->wave.scan_hi, m1);
}

// Pass A again from message 0 over the resident messages [0, n) of the wave in flight (scratch sized for `cap`):
// after the store widened (finish_wave_elastic), or for the prefix of a node wave cut at n (pnc_node_prefix).
void rescan_wave(jg_pnc* p, const uint8_t* bytes, const uint64_t* off, const uint32_t* rows, uint64_t n, uint64_t cap) {
    const WaveScratch w = wave_scratch(p, cap);
    begin_status(p, w.status);
    p->wave.scan_hi = 0;
    launch_scan(p, bytes, off, rows, 0, n, w);
}

// A fused pass A over messages [0, p->wave.scan_hi) taken back (stream-ordered): the wave failed after it, or a node
// wave was cut or aborted.  Idempotent; a no-op for messages pass A left to pass B.
void undo_applied(jg_pnc* p, const uint32_t* rows) {
    const uint64_t n = p->wave.scan_hi;
    if (n == 0 || !p->wave.emit.p) return;
    const Table t = table_of(p);
    const unsigned g = blocks_for(n * kEmitLanes);
    jg::dispatch_eb(p->eb, [&](auto EB) {
        hipLaunchKernelGGL(k_undo_applied<EB()>, dim3(g), dim3(kBlock), 0, p->ctx->stream, p->wave.emit.as<uint8_t>(), rows, n, t.R, p->rw_P(), p->rw_N());
    });
    JG_HIP(hipGetLastError());
}

// After pass A over all n messages: check, resolve new replicas, apply.  All or nothing.
void finish_wave(jg_pnc* p, const uint8_t* bytes, const uint64_t* off, const uint32_t* rows, uint64_t n, const WaveScratch& w,
                 uint64_t* bad_msg) {
    jg_ctx* ctx = p->ctx;
    const Table t = table_of(p);
    const int G = json_group();
    const unsigned ge = blocks_for(n * kEmitLanes);
    if (G > 1) {
        // The steady state of a fused wave (every payload compact and valid, every replica known): pass A's status
        // alone ends it — one read, no slow-list launches (round 6: k_scan_slow and k_apply_slow cost ~5 µs each
        // even with nothing to do, the next wave's status reset another 5).  Otherwise the launches below.
        if (p->wave.fuse) {
            const Status s0 = read_status(ctx, w.status);
            if (s0.first_bad == ~0ull && s0.n_deferred == 0 && s0.resolve_bad == ~0ull && s0.n_slow == 0 && s0.n_resume == 0) {
                p->wave.status_clean = true;
                return;
            }
        }
        // the payloads the group parse left to the serial parser (count read on the device)
        jg::dispatch_eb(p->eb, [&](auto EB) {
            hipLaunchKernelGGL(k_scan_slow<EB()>, dim3(64), dim3(kBlock), 0, ctx->stream, bytes, off, rows, t, w.status, w.deferred, w.emit, w.slow);
        });
        JG_HIP(hipGetLastError());
        // The steady state (every payload valid, every replica known): pass B right away, guarded on the
        // device by pass A's status, so the wave costs one status read.  If pass A failed or deferred a
        // message both launches are no-ops and the full path below runs (all or nothing).  A fused pass A
        // (jg::PncWave::fuse) applied every record pass B would read here (a deferral sends the wave to the full path,
        // whose pass B runs unguarded): only the slow list's launch is left.
        const bool fused = p->wave.fuse;
        jg::dispatch_eb(p->eb, [&](auto EB) {
            if (!fused) hipLaunchKernelGGL(k_apply_emit<EB()>, dim3(ge), dim3(kBlock), 0, ctx->stream, w.emit, rows, n, t.R, p->rw_P(), p->rw_N(), w.status);
            hipLaunchKernelGGL(k_apply_slow<EB()>, dim3(64), dim3(kBlock), 0, ctx->stream, bytes, off, rows, w.slow, t, p->rw_P(), p->rw_N(), w.status);
        });
        JG_HIP(hipGetLastError());
        const Status st = read_status(ctx, w.status);
        if (st.first_bad != ~0ull) undo_applied(p, rows), fail_msg(st.first_bad, bad_msg, "state message");
        if (!st.n_deferred) {
            // only k_apply_slow can have set it here (no walk ran): kErrInternal, a JG_EHIP without a cut; the
            // fused applies are taken back, the slow list's raises (no undo records) stay — an internal failure
            if (st.resolve_bad != ~0ull) undo_applied(p, rows), fail_msg(st.resolve_bad, bad_msg, "state message");
            return;
        }
    }
    DeferredLists dl = select_deferred(ctx, w.deferred, n, p->n_keys, w.status + 1);
    Status st = read_status(ctx, w.status);
    if (st.first_bad != ~0ull) undo_applied(p, rows), fail_msg(st.first_bad, bad_msg, "state message");
    unsigned long long* sorted_deferred = nullptr;
    if (st.n_deferred) {
        const uint64_t nd = st.n_deferred;
        unsigned long long* sorted = sort_deferred(ctx, dl, nd);
        sorted_deferred = sorted;
        const unsigned gd = blocks_for(nd);
        // the resume list reuses pass A's deferral marks (dead once compacted)
        jg::dispatch_eb(p->eb, [&](auto EB) {
            launch_resolve_g<EB()>(G, ctx->stream, bytes, off, sorted, nd, t, w.emit, w.eguid, w.saved, w.status, w.deferred);
        });
        JG_HIP(hipGetLastError());
        st = read_status(ctx, w.status);
        if (st.n_resume && st.resolve_bad == ~0ull) {  // walks the group parse handed to the serial parser
            jg::dispatch_eb(p->eb, [&](auto EB) {
                hipLaunchKernelGGL(k_resolve_resume<EB()>, dim3(64), dim3(kBlock), 0, ctx->stream, bytes, off, sorted, nd, t, w.status, w.deferred, w.emit,
                                   w.eguid);
            });
            JG_HIP(hipGetLastError());
            st = read_status(ctx, w.status);
        }
        if (st.resolve_bad != ~0ull) {
            hipLaunchKernelGGL(k_rollback, dim3(gd), dim3(kBlock), 0, ctx->stream, sorted, nd, t, w.saved);
            JG_HIP(hipGetLastError());
            undo_applied(p, rows);
            JG_HIP(hipStreamSynchronize(ctx->stream));
            fail_msg(st.resolve_bad, bad_msg, "state message");
        }
    }
    // pass B: pass A's records (resolved by pass C where deferred), then the messages left to the serial
    // parser (slow: not in the compact form; with JANUS_JSON_GROUP=1 also the deferred ones).  max is
    // order-free.
    jg::dispatch_eb(p->eb, [&](auto EB) {
        hipLaunchKernelGGL(k_apply_emit<EB()>, dim3(ge), dim3(kBlock), 0, ctx->stream, w.emit, rows, n, t.R, p->rw_P(), p->rw_N(), nullptr);
    });
    JG_HIP(hipGetLastError());
    const unsigned long long* lists[2] = {st.n_deferred ? sorted_deferred : nullptr, w.slow};
    const uint64_t counts[2] = {st.n_deferred, st.n_slow};
    for (int l = G > 1 ? 1 : 0; l < 2; ++l) {
        if (!counts[l]) continue;
        const unsigned gl = blocks_for(counts[l]);
        jg::dispatch_eb(p->eb, [&](auto EB) {
            hipLaunchKernelGGL(k_apply_list<EB()>, dim3(gl), dim3(kBlock), 0, ctx->stream, bytes, off, rows, lists[l], counts[l], t, p->rw_P(), p->rw_N(), w.status);
        });
        JG_HIP(hipGetLastError());
    }
    st = read_status(ctx, w.status);
    // Past pass C every message has been judged, so only k_apply_list's re-parse (apply_one: kErrInternal) can set
    // it now: the library's own inconsistency, raised as JG_EHIP without naming a message (fail_msg), so it is never
    // taken for a cut whose prefix re-run would leave pass B's raises (no undo records) in the store.
    if (st.resolve_bad != ~0ull) {
        JG_REQUIRE((st.resolve_bad & 3) == kErrInternal, JG_EHIP, "pass B: status %llx after every message was judged", st.resolve_bad);
        undo_applied(p, rows);
        fail_msg(st.resolve_bad, bad_msg, "state message");
    }
}

// finish_wave for a store that may widen itself (jg_pnc_set_max_replicas; a fixed store takes the plain call and
// its errors).  A wave that fails for row capacity has been rolled back whole — the columns it added and the fused
// pass A's raises — so the store holds its contents from before the wave: widen it (the contents padded with
// zeros), run pass A again over the same resident messages [0, n) at the new stride, and finish again; until the
// wave is through or R stands at its bound, where the failure is the fixed store's (same code, same *bad_msg).
// `cap` = the messages the wave's scratch was sized for.
void finish_wave_elastic(jg_pnc* p, const uint8_t* bytes, const uint64_t* off, const uint32_t* rows, uint64_t n, uint64_t cap,
                         uint64_t* bad_msg) {
    for (;;) {
        try {
            finish_wave(p, bytes, off, rows, n, wave_scratch(p, cap), bad_msg);
            return;
        } catch (const RowFull&) {
            if (!jg::pnc_auto_widen(p)) throw;
        }
        if (bad_msg) *bad_msg = UINT64_MAX;
        rescan_wave(p, bytes, off, rows, n, cap);
    }
}

// The whole device side of a wave already in device memory.
void merge_wave_dev(jg_pnc* p, const uint8_t* bytes, const uint64_t* off, const uint32_t* rows, uint64_t n, uint64_t* bad_msg) {
    launch_scan(p, bytes, off, rows, 0, n, begin_wave(p, n));
    finish_wave_elastic(p, bytes, off, rows, n, n, bad_msg);
}

void check_wave_host(const jg_pnc* p, uint64_t n, const uint32_t* key_idx, const uint64_t* off, const char* fn) {
    JG_REQUIRE(n < 0xFFFFFFFFull, JG_EINVAL, "%s: at most 2^32-2 messages per wave", fn);
    JG_REQUIRE(off[0] == 0, JG_EINVAL, "%s: off[0] must be 0", fn);
    for (uint64_t i = 0; i < n; ++i) {
        JG_REQUIRE(off[i + 1] >= off[i], JG_EINVAL, "%s: offsets decrease at message %llu", fn, (unsigned long long)i);
        JG_REQUIRE(key_idx[i] < p->n_keys, JG_EINVAL, "%s: key_idx[%llu] = %u out of range (n_keys %llu)", fn, (unsigned long long)i,
                   key_idx[i], (unsigned long long)p->n_keys);
    }
}

}  // namespace

// ---- node waves (csrc/node.hip) ------------------------------------------------------------------
// The node uploads every kind's messages of a committed wave once, classifies them on the device and
// drives this path over its own buffers: rows[m] = the message's row, or kSkipIdx for another kind's.
namespace jg {

void pnc_node_begin(jg_pnc* p, uint64_t n) {
    begin_wave(p, n);
    p->wave.n = n;  // the node wave's capacity (jg_pnc_wave_* calls are refused while it is open: node_open)
}

void pnc_node_scan(jg_pnc* p, const uint8_t* bytes, const uint64_t* off, const uint32_t* rows, uint64_t m0, uint64_t m1) {
    launch_scan(p, bytes, off, rows, m0, m1, wave_scratch(p, p->wave.n));
}

// The rest of the wave over messages [0, n) (pass A ran on all of them), all or nothing: JG_OK, or the
// code of the first rejected message (*bad, why) with nothing applied.  Other failures throw.
int pnc_node_finish(jg_pnc* p, const uint8_t* bytes, const uint64_t* off, const uint32_t* rows, uint64_t n, uint64_t* bad, std::string* why) {
    *bad = UINT64_MAX;
    if (n == 0) return JG_OK;
    try {
        // a store that widens itself (jg_pnc_set_max_replicas) runs the resident messages again instead of cutting
        // the wave at a key that ran out of columns; the widening passes the node wave's hold on the store
        finish_wave_elastic(p, bytes, off, rows, n, p->wave.n, bad);
        p->wave.scan_hi = 0;  // committed: a later abort of the node wave (an OR-Set commit failing) must not undo it
        return JG_OK;
    } catch (const Error& e) {
        if (*bad == UINT64_MAX) throw;
        *why = e.msg;
        return e.code;
    }
}

// Pass A again over [0, n) only, then the rest: the prefix of a wave cut at n (the reference's loop
// applied the messages before the one that threw).
int pnc_node_prefix(jg_pnc* p, const uint8_t* bytes, const uint64_t* off, const uint32_t* rows, uint64_t n, uint64_t* bad, std::string* why) {
    *bad = UINT64_MAX;
    undo_applied(p, rows);  // the chunks' fused pass A applied messages past the cut too: back to the state before the wave
    p->wave.scan_hi = 0;
    if (n == 0) return JG_OK;  // a cut at message 0: nothing applied (the undo used to come after this return)
    rescan_wave(p, bytes, off, rows, n, p->wave.n);
    return pnc_node_finish(p, bytes, off, rows, n, bad, why);
}

// A node wave abandoned after its chunks' pass A (an internal failure): the fused applies taken back.
void pnc_node_undo(jg_pnc* p, const uint32_t* rows) {
    undo_applied(p, rows);
    p->wave.scan_hi = 0;
}

PncTable pnc_replica_table(jg_pnc* p) {
    ensure_table(p);
    return PncTable{p->cols.as<unsigned long long>(), p->ncols.as<uint32_t>(), p->R};
}

}  // namespace jg

// Device-resident wave of encoded state messages (bench / pre-staged waves).
extern "C" {

int jg_pnc_intern(jg_pnc* p, uint64_t n, const uint32_t* key_idx, const jg_guid* replica, uint32_t* col_out) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        jg::require_writable(p, "jg_pnc_intern");
        JG_REQUIRE(p, JG_EINVAL, "jg_pnc_intern: store is NULL");
        if (n == 0) return;
        JG_REQUIRE(key_idx && replica && col_out, JG_EINVAL, "jg_pnc_intern: NULL argument");
        JG_REQUIRE(n < 0xFFFFFFFFull, JG_EINVAL, "jg_pnc_intern: at most 2^32-2 entries per call");
        for (uint64_t i = 0; i < n; ++i)
            JG_REQUIRE(key_idx[i] < p->n_keys, JG_EINVAL, "jg_pnc_intern: key_idx[%llu] = %u out of range", (unsigned long long)i, key_idx[i]);
        jg_ctx* ctx = p->ctx;
        jg::ensure_device(ctx);
        ensure_table(p);
        unsigned long long *status, *keys;
        Guid16* g;
        uint32_t *rows, *cols, *saved;
        jg::Layout L;
        L.add(status, 8, 64), L.add(keys, n, 8), L.add(g, n, 8), L.add(rows, n, 4), L.add(cols, n, 4), L.add(saved, n, 4);
        L.bind(jg::scratch(ctx, ctx->scratch, L.bytes() + 256));
        JG_HIP(hipMemcpyAsync(rows, key_idx, n * 4, hipMemcpyHostToDevice, ctx->stream));
        JG_HIP(hipMemcpyAsync(g, replica, n * 16, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_make_keys<false>, dim3(blocks_for(n)), dim3(kBlock), 0, ctx->stream, rows, n, keys);
        unsigned long long* sorted = sort_keys(ctx, keys, n, p->n_keys);
        for (;;) {  // once, or again on a wider store while it may widen itself (jg_pnc_set_max_replicas)
            const Table t = table_of(p);
            reset_status(ctx, status);
            hipLaunchKernelGGL(k_intern, dim3(blocks_for(n)), dim3(kBlock), 0, ctx->stream, sorted, n, g, t, cols, saved, status);
            JG_HIP(hipGetLastError());
            const Status st = read_status(ctx, status);
            if (st.resolve_bad == ~0ull) break;
            hipLaunchKernelGGL(k_rollback, dim3(blocks_for(n)), dim3(kBlock), 0, ctx->stream, sorted, n, t, saved);
            JG_HIP(hipStreamSynchronize(ctx->stream));
            if (jg::pnc_auto_widen(p)) continue;  // rolled back: the same entries over the wider rows
            jg::fail(JG_ESTATE, "jg_pnc_intern: entry %llu: its key holds more replicas than the store's columns",
                     (unsigned long long)(st.resolve_bad >> 2));
        }
        JG_HIP(hipMemcpyAsync(col_out, cols, n * 4, hipMemcpyDeviceToHost, ctx->stream));
        JG_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int jg_pnc_columns(jg_pnc* p, uint64_t n, const uint32_t* key_idx, jg_guid* replicas, uint32_t* ncols) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        JG_REQUIRE(p, JG_EINVAL, "jg_pnc_columns: store is NULL");
        if (n == 0) return;
        JG_REQUIRE(key_idx && replicas && ncols, JG_EINVAL, "jg_pnc_columns: NULL argument");
        for (uint64_t i = 0; i < n; ++i)
            JG_REQUIRE(key_idx[i] < p->n_keys, JG_EINVAL, "jg_pnc_columns: key_idx[%llu] = %u out of range", (unsigned long long)i, key_idx[i]);
        jg_ctx* ctx = p->ctx;
        jg::ensure_device(ctx);
        ensure_table(p);
        uint32_t *rows, *nout;
        Guid16* out;
        jg::Layout L;
        L.add(rows, n, 4), L.add(nout, n, 4), L.add(out, n * p->R, 16);
        L.bind(jg::scratch(ctx, ctx->scratch, L.bytes() + 256));
        JG_HIP(hipMemcpyAsync(rows, key_idx, n * 4, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_gather_cols, dim3(blocks_for(n * p->R)), dim3(kBlock), 0, ctx->stream, p->cols.as<Guid16>(), p->ncols.as<uint32_t>(),
                           rows, n, p->R, out, nout);
        JG_HIP(hipGetLastError());
        JG_HIP(hipMemcpyAsync(replicas, out, n * 16ull * p->R, hipMemcpyDeviceToHost, ctx->stream));
        JG_HIP(hipMemcpyAsync(ncols, nout, n * 4, hipMemcpyDeviceToHost, ctx->stream));
        JG_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int jg_wave_create(jg_ctx* ctx, uint64_t cap_msgs, uint64_t cap_bytes, jg_wave** out) {
    return jg::guard([&] {
        auto lk_ = jg::lock(ctx);  // calls on one context are serialised (shared scratch, stream)
        JG_REQUIRE(ctx && out, JG_EINVAL, "jg_wave_create: NULL argument");
        JG_REQUIRE(cap_msgs < 0xFFFFFFFFull, JG_EINVAL, "jg_wave_create: at most 2^32-2 messages per wave");
        jg::ensure_device(ctx);
        auto* w = new jg_wave();
        w->ctx = ctx;
        w->cap_msgs = cap_msgs;
        w->cap_bytes = cap_bytes;
        try {
            w->bytes.alloc(jg::round_up(cap_bytes, 16) + 16);  // the parser reads aligned 16-byte windows
            w->off.alloc((cap_msgs + 1) * 8);
            w->keys.alloc(cap_msgs * 4 + 4);
        } catch (...) {
            delete w;
            throw;
        }
        *out = w;
    });
}

int jg_wave_destroy(jg_wave* w) {
    return jg::guard([&] {
        auto lk_ = jg::lock(w);  // calls on one context are serialised (shared scratch, stream)
        if (!w) return;
        jg::ensure_device(w->ctx);
        JG_HIP(hipStreamSynchronize(w->ctx->stream));
        delete w;
    });
}

int jg_wave_upload(jg_wave* w, uint64_t n, const uint32_t* key_idx, const uint64_t* off, const uint8_t* bytes) {
    return jg::guard([&] {
        auto lk_ = jg::lock(w);  // calls on one context are serialised (shared scratch, stream)
        JG_REQUIRE(w && key_idx && off && (bytes || n == 0), JG_EINVAL, "jg_wave_upload: NULL argument");
        JG_REQUIRE(n <= w->cap_msgs && off[n] <= w->cap_bytes, JG_EINVAL, "jg_wave_upload: wave exceeds the capacity");
        JG_REQUIRE(off[0] == 0, JG_EINVAL, "jg_wave_upload: off[0] must be 0");
        uint32_t mx = 0;
        for (uint64_t i = 0; i < n; ++i) {
            JG_REQUIRE(off[i + 1] >= off[i], JG_EINVAL, "jg_wave_upload: offsets decrease at message %llu", (unsigned long long)i);
            mx = key_idx[i] > mx ? key_idx[i] : mx;
        }
        jg_ctx* ctx = w->ctx;
        jg::ensure_device(ctx);
        if (off[n]) JG_HIP(hipMemcpyAsync(w->bytes.p, bytes, off[n], hipMemcpyHostToDevice, ctx->stream));
        JG_HIP(hipMemcpyAsync(w->off.p, off, (n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        if (n) JG_HIP(hipMemcpyAsync(w->keys.p, key_idx, n * 4, hipMemcpyHostToDevice, ctx->stream));
        JG_HIP(hipStreamSynchronize(ctx->stream));
        w->n = n;
        w->n_bytes = off[n];
        w->max_key = mx;
    });
}

int jg_pnc_merge_wave(jg_pnc* p, const jg_wave* w, uint64_t* bad_msg) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        jg::require_writable(p, "jg_pnc_merge_wave");
        if (bad_msg) *bad_msg = UINT64_MAX;
        JG_REQUIRE(p && w, JG_EINVAL, "jg_pnc_merge_wave: NULL argument");
        JG_REQUIRE(p->ctx == w->ctx, JG_EINVAL, "jg_pnc_merge_wave: wave and store belong to different contexts");
        if (w->n == 0) return;
        JG_REQUIRE(w->max_key < p->n_keys, JG_EINVAL, "jg_pnc_merge_wave: wave addresses key %u >= n_keys %llu", w->max_key,
                   (unsigned long long)p->n_keys);
        jg::ensure_device(p->ctx);
        merge_wave_dev(p, w->bytes.as<uint8_t>(), w->off.as<uint64_t>(), w->keys.as<uint32_t>(), w->n, bad_msg);
    });
}

int jg_pnc_wave_begin(jg_pnc* p, uint64_t cap_msgs, uint64_t cap_bytes) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        jg::require_writable(p, "jg_pnc_wave_begin");
        JG_REQUIRE(p, JG_EINVAL, "jg_pnc_wave_begin: store is NULL");
        jg_ctx* ctx = p->ctx;
        jg::ensure_device(ctx);
        ensure_table(p);  // ahead of the buffers, as ever (begin_wave's own call then finds it there)
        grow_keep(ctx, p->wave.bytes, jg::round_up(cap_bytes, 16) + 16, 0);
        grow_keep(ctx, p->wave.off, (cap_msgs + 1) * 8, 0);
        grow_keep(ctx, p->wave.rows, cap_msgs * 4 + 4, 0);
        begin_wave(p, cap_msgs);
        JG_HIP(hipMemsetAsync(p->wave.off.p, 0, 8, ctx->stream));  // off[0] = 0
        p->wave.n = 0;
        p->wave.nb = 0;
        p->wave.open = true;
    });
}

int jg_pnc_wave_append(jg_pnc* p, uint64_t n, const uint32_t* key_idx, const uint64_t* off, const uint8_t* bytes) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        jg::require_writable(p, "jg_pnc_wave_append");
        JG_REQUIRE(p && p->wave.is_open(), JG_EINVAL, "jg_pnc_wave_append: no open wave (jg_pnc_wave_begin)");
        if (n == 0) return;
        JG_REQUIRE(key_idx && off && bytes, JG_EINVAL, "jg_pnc_wave_append: NULL argument");
        check_wave_host(p, n, key_idx, off, "jg_pnc_wave_append");
        JG_REQUIRE(p->wave.n + n < 0xFFFFFFFFull, JG_EINVAL, "jg_pnc_wave_append: at most 2^32-2 messages per wave");
        jg_ctx* ctx = p->ctx;
        jg::ensure_device(ctx);
        const uint64_t m0 = p->wave.n, b0 = p->wave.nb, nb = off[n];
        // grow (rare: the caller's capacity hint was short); earlier chunks are kept
        if (p->wave.bytes.bytes < jg::round_up(b0 + nb, 16) + 16 || p->wave.off.bytes < (m0 + n + 1) * 8 || p->wave.rows.bytes < (m0 + n) * 4 + 4) {
            const uint64_t need_m = 2 * (m0 + n), need_b = 2 * (b0 + nb);
            grow_keep(ctx, p->wave.bytes, jg::round_up(need_b, 16) + 16, b0);
            grow_keep(ctx, p->wave.off, (need_m + 1) * 8, (m0 + 1) * 8);
            grow_keep(ctx, p->wave.rows, need_m * 4 + 4, m0 * 4);
        }
        const WaveScratch w = wave_scratch(p, m0 + n, m0);  // keeps the entries earlier chunks deferred
        if (nb) JG_HIP(hipMemcpyAsync(p->wave.bytes.as<uint8_t>() + b0, bytes, nb, hipMemcpyHostToDevice, ctx->stream));
        JG_HIP(hipMemcpyAsync(p->wave.off.as<uint64_t>() + m0 + 1, off + 1, n * 8, hipMemcpyHostToDevice, ctx->stream));
        JG_HIP(hipMemcpyAsync(p->wave.rows.as<uint32_t>() + m0, key_idx, n * 4, hipMemcpyHostToDevice, ctx->stream));
        if (b0) hipLaunchKernelGGL(k_rebase, dim3(blocks_for(n)), dim3(kBlock), 0, ctx->stream, p->wave.off.as<uint64_t>() + m0 + 1, n, b0);
        launch_scan(p, p->wave.bytes.as<uint8_t>(), p->wave.off.as<uint64_t>(), p->wave.rows.as<uint32_t>(), m0, m0 + n, w);
        p->wave.n = m0 + n;
        p->wave.nb = b0 + nb;
    });
}

int jg_pnc_wave_commit(jg_pnc* p, uint64_t* bad_msg) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        jg::require_writable(p, "jg_pnc_wave_commit");
        if (bad_msg) *bad_msg = UINT64_MAX;
        JG_REQUIRE(p && p->wave.is_open(), JG_EINVAL, "jg_pnc_wave_commit: no open wave (jg_pnc_wave_begin)");
        jg::ensure_device(p->ctx);
        p->wave.open = false;
        if (p->wave.n == 0) return;
        finish_wave_elastic(p, p->wave.bytes.as<uint8_t>(), p->wave.off.as<uint64_t>(), p->wave.rows.as<uint32_t>(), p->wave.n, p->wave.n, bad_msg);
    });
}

int jg_pnc_wave_abort(jg_pnc* p) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        jg::require_writable(p, "jg_pnc_wave_abort");
        JG_REQUIRE(p, JG_EINVAL, "jg_pnc_wave_abort: store is NULL");
        jg::ensure_device(p->ctx);
        if (p->wave.is_open()) undo_applied(p, p->wave.rows.as<uint32_t>());  // the appended chunks' fused pass A
        p->wave.scan_hi = 0;
        JG_HIP(hipStreamSynchronize(p->ctx->stream));
        p->wave.open = false;
    });
}

int jg_pnc_merge_json(jg_pnc* p, uint64_t n, const uint32_t* key_idx, const uint64_t* off, const uint8_t* bytes, uint64_t* bad_msg) {
    auto lk_ = jg::lock(p);  // the whole begin/append/commit sequence under the context lock
    if (bad_msg) *bad_msg = UINT64_MAX;
    if (p && n && off) {
        int rc = jg_pnc_wave_begin(p, n, off[n]);
        if (rc == JG_OK) rc = jg_pnc_wave_append(p, n, key_idx, off, bytes);
        if (rc != JG_OK) {
            char keep[1024];
            jg_last_error(keep, sizeof keep);
            jg_pnc_wave_abort(p);
            return jg::guard([&] { jg::fail(rc, "%s", keep); });
        }
        return jg_pnc_wave_commit(p, bad_msg);
    }
    return jg::guard([&] {
        JG_REQUIRE(p, JG_EINVAL, "jg_pnc_merge_json: store is NULL");
        JG_REQUIRE(n == 0, JG_EINVAL, "jg_pnc_merge_json: NULL argument");
    });
}

}  // extern "C"
