// adopt.hip — CRDT creation on the device: jg_node_create_uids (a batch of ReplicationManager.ReceivedNewObjectSyncMsg,
// BFT-CRDT/ReplicationManager.cs:310-324), jg_node_adopt_keys (KeySpaceManager.OnNext's CreateSafeCRDT(key, guid) for
// journalled keys, KeySpaceManager.cs:151-178 -> SafeCRDTManager.cs:86-101) and jg_node_next_idx.  The node allocates
// the rows and set ids; the caller keeps no allocator and no uid -> (type, row) map.
//
// One batch of n items (the call's uids, or journal records [from, to) read where keyspace.hip left them) goes
//   k_resolve   one lane per item (adopt: after k_journal_uids copied the records' Guids): the journal status, the kind from the prospective copy's uid table (adopt), the uid in
//               the node's own table (uid_find); an item the table lacks claims its uid in a call-wide table
//               (tpset_dict.hpp claim_slot) and takes atomicMin of its index there: the first occurrence wins
//   k_rank      winner flags per kind (what jgt::excl_scan ranks)
//   two scans   rank of every winner among its kind's, in call order; the kinds' totals
//   k_assign    row = next_row + rank | set id = next_set + rank; a loser reads its winner's; statuses, kinds and
//               indices as the call reports them; a replica that finds no free column in an existing row raises a flag
//   (totals and flags read back: the refusals, the store's growth — nothing has been written so far)
//   k_commit    winners claim a free slot of the node's table (uid_claim) and write their entry; a PN-Counter winner
//               interns its replica in its row
// and the (slot, entry) pairs come back for the host copy of the table (node_insert_commit: no second probe).
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tpset_host.hpp"
#include "uid_table.hpp"

namespace {

using jg::DevUids;
using jg::kNoSlot;
using jg::kOrSetBit;
using jg::UidSlot;
using jgt::ull;

constexpr uint32_t kLanes = 256;
// an item before its rank is known: it may create its uid (0), the node holds the uid (1), or it has one of the two
// statuses that never create (JG_A_NO_TYPE, JG_A_SKIPPED: their own codes)
enum : uint8_t { kCandidate = 0, kHeld = 1 };
static_assert(JG_A_NO_TYPE > kHeld && JG_A_SKIPPED > kHeld && JG_C_CREATED == JG_A_ADOPTED && JG_C_EXISTS == JG_A_HAVE, "one status rule for both calls");
enum : ull { kFlagNoPnc = 1, kFlagNoOrset = 2, kFlagRowFull = 4 };

struct Items {
    uint64_t n;
    jg_guid* uid;      // the item's uid (adopt: copied out of the journal, k_journal_uids)
    jg_guid* replica;  // NULL: nothing interned
    uint8_t *code, *kind;
    uint32_t *held, *cslot, *prep, *pmin;  // held: the table's val of a uid the node holds
    uint64_t pmask;
    uint32_t *wp, *ws;  // 1: the item creates a PN-Counter / an OR-Set
    ull *op, *os;       // their exclusive scans, [n + 1]
    ull* flags;
    // as reported
    uint8_t *status, *okind;
    uint32_t *idx, *slot, *val;
};

struct SameUid {
    const jg_guid* uid;
    ull lo, hi;
    __device__ bool operator()(uint32_t o) const { return uid[o].lo == lo && uid[o].hi == hi; }
};

// journal records from `from` as the call's uids (a launch of its own: k_resolve's lanes compare one another's uids)
__global__ __launch_bounds__(kLanes) void k_journal_uids(Items I, const ull* __restrict__ jglo, const ull* __restrict__ jghi, uint64_t from) {
    const uint64_t i = (uint64_t)blockIdx.x * kLanes + threadIdx.x;
    if (i < I.n) I.uid[i] = jg_guid{jglo[from + i], jghi[from + i]};
}

// type: the call's kinds (create) or NULL (adopt: the journal's statuses from `from`, the kind read from `prosp`)
__global__ __launch_bounds__(kLanes) void k_resolve(Items I, const uint8_t* __restrict__ type, const uint8_t* __restrict__ jstatus, uint64_t from,
                                                    DevUids prosp, DevUids own) {
    const uint64_t i = (uint64_t)blockIdx.x * kLanes + threadIdx.x;
    if (i >= I.n) return;
    uint8_t code = kCandidate, kind = 255;
    uint32_t held = kNoSlot, cslot = kNoSlot;
    const ull lo = I.uid[i].lo, hi = I.uid[i].hi;
    if (type) {
        kind = type[i];
    } else {
        if (jstatus[from + i] != 0) {
            code = JG_A_SKIPPED;
        } else {
            const uint32_t pv = jg::uid_find(prosp, lo, hi);  // Guid.Empty is never registered: NO_TYPE
            if (pv == kNoSlot) code = JG_A_NO_TYPE;
            else kind = pv >> 31;
        }
    }
    if (code == kCandidate) {
        held = jg::uid_find(own, lo, hi);
        if (held != kNoSlot) {
            code = kHeld;
        } else {
            cslot = jgt::claim_slot(I.prep, I.pmask, jg::uid_hash(lo, hi), (uint32_t)i, SameUid{I.uid, lo, hi});
            atomicMin(&I.pmin[cslot], (uint32_t)i);
        }
    }
    I.code[i] = code, I.kind[i] = kind, I.held[i] = held, I.cslot[i] = cslot;
}

__global__ __launch_bounds__(kLanes) void k_rank(Items I) {
    const uint64_t i = (uint64_t)blockIdx.x * kLanes + threadIdx.x;
    if (i >= I.n) return;
    const bool win = I.code[i] == kCandidate && I.pmin[I.cslot[i]] == (uint32_t)i;
    I.wp[i] = win && I.kind[i] == 0, I.ws[i] = win && I.kind[i] == 1;
}

// has: bit 0 the node has a PN-Counter store, bit 1 an OR-Set store.  cols / ncols / R / n_keys: the replica table as it
// stands (rows from n_keys on do not exist yet and are fresh once they do).
__global__ __launch_bounds__(kLanes) void k_assign(Items I, uint32_t next_row, uint32_t next_set, uint32_t has, const jg_guid* __restrict__ cols,
                                                   const uint32_t* __restrict__ ncols, uint32_t R, uint64_t n_keys) {
    const uint64_t i = (uint64_t)blockIdx.x * kLanes + threadIdx.x;
    if (i >= I.n) return;
    const uint8_t code = I.code[i];
    uint8_t status = code, kind = 255;
    uint32_t idx = 0xFFFFFFFFu, val = kNoSlot;
    if (code == kHeld) {
        const uint32_t v = I.held[i];
        kind = v >> 31, idx = v & ~kOrSetBit, status = JG_C_EXISTS;
    } else if (code == kCandidate) {
        const uint32_t w = I.pmin[I.cslot[i]];  // the first item of this uid: its kind decides, its rank is the index
        kind = I.kind[w];
        idx = kind ? next_set + (uint32_t)I.os[w] : next_row + (uint32_t)I.op[w];
        status = w == (uint32_t)i ? JG_C_CREATED : JG_C_EXISTS;
        if (w == (uint32_t)i) {
            val = kind ? idx | kOrSetBit : idx;
            if (!(has >> kind & 1)) atomicOr(I.flags, kind ? kFlagNoOrset : kFlagNoPnc);
            if (kind == 0 && I.replica && idx < n_keys && ncols[idx] >= R) {  // a row someone interned by hand, full
                const jg_guid g = I.replica[i];
                bool found = false;
                for (uint32_t c = 0; c < R; ++c) found |= cols[(uint64_t)idx * R + c].lo == g.lo && cols[(uint64_t)idx * R + c].hi == g.hi;
                if (!found) atomicOr(I.flags, kFlagRowFull);
            }
        }
    }
    I.status[i] = status, I.okind[i] = kind, I.idx[i] = idx, I.val[i] = val;
}

// cols / ncols NULL: no replica is interned.  Winners hold distinct rows, so a row has one writer.
__global__ __launch_bounds__(kLanes) void k_commit(Items I, UidSlot* __restrict__ tab, uint64_t mask, jg_guid* __restrict__ cols, uint32_t* __restrict__ ncols,
                                                   uint32_t R) {
    const uint64_t i = (uint64_t)blockIdx.x * kLanes + threadIdx.x;
    if (i >= I.n) return;
    const uint32_t val = I.val[i];
    uint32_t slot = kNoSlot;
    if (val != kNoSlot) {
        const jg_guid u = I.uid[i];
        slot = jg::uid_claim(tab, mask, u.lo, u.hi);
        tab[slot].lo = u.lo, tab[slot].hi = u.hi, tab[slot].val = val;
        if (cols && !(val & kOrSetBit)) {
            const jg_guid g = I.replica[i];
            jg_guid* row = cols + (uint64_t)val * R;
            const uint32_t nc = ncols[val];
            uint32_t c = 0;
            while (c < nc && !(row[c].lo == g.lo && row[c].hi == g.hi)) ++c;
            if (c == nc && nc < R) row[nc] = g, ncols[val] = nc + 1;  // (nc == R was refused: k_assign's flag)
        }
    }
    I.slot[i] = slot;
}

struct Call {
    const char* fn;
    jg_node* node;
    uint64_t n;
    // create
    const jg_guid* uid = nullptr;
    const uint8_t* type = nullptr;
    // adopt
    jg_node* prospective = nullptr;
    jg_keyspace* ks = nullptr;
    uint64_t from = 0;
    const jg_guid* replica = nullptr;
    uint64_t max_keys = 0;
    uint8_t *status = nullptr, *kind = nullptr;
    uint32_t* idx = nullptr;
};

// JANUS_TRACE_ADOPT (as JANUS_TRACE_QUERY): the call's launches by hipEvents, to stderr
struct Trace {
    static constexpr int kMax = 8;
    bool on;
    hipStream_t st;
    hipEvent_t ev[kMax] = {};
    const char* what[kMax] = {};
    int k = 0;
    void stamp(const char* w) {
        if (!on || k == kMax) return;
        JG_HIP(hipEventCreate(&ev[k]));
        JG_HIP(hipEventRecord(ev[k], st));
        what[k++] = w;
    }
    void print(const char* fn, uint64_t n) {
        if (!on) return;
        std::fprintf(stderr, "%s(%llu items):", fn, (ull)n);
        for (int j = 1; j < k; ++j) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, ev[j - 1], ev[j]) != hipSuccess) (void)hipGetLastError();  // a host wait lay between the two
            std::fprintf(stderr, " %s %.3f ms%s", what[j], ms, j + 1 < k ? "," : "\n");
        }
    }
    ~Trace() {
        for (int j = 0; j < k; ++j) (void)hipEventDestroy(ev[j]);
    }
};

void run(const Call& c) {
    const uint64_t n = c.n;
    const bool adopt = c.ks != nullptr;
    jg_ctx* ctx = jg::node_ctx(c.node);
    jg::ensure_device(ctx);
    // the node's table with room for every item, then the prospective copy's (the same node: its table as just grown)
    const jg::NodeInsert nd = jg::node_insert_begin(c.node, n, c.fn);
    DevUids prosp{nullptr, 0};
    if (adopt) prosp = jg::node_query_ref(c.prospective, c.fn).uids;
    if (!adopt)
        for (uint64_t i = 0; i < n; ++i)
            JG_REQUIRE(c.type[i] ? nd.orset != nullptr : nd.pnc != nullptr, JG_EINVAL, "%s: entry %llu is %s but the node has no such store", c.fn, (ull)i,
                       c.type[i] ? "an ORSet" : "a PNCounter");
    const bool intern = c.replica && nd.pnc;
    jg::PncTable T{nullptr, nullptr, 0};
    if (intern) T = jg::pnc_replica_table(nd.pnc);
    hipStream_t st = ctx->stream;

    Items I{};
    uint8_t* d_type = nullptr;
    const uint64_t slots = jg::pow2_at_least(2 * n, 64);
    jg::Layout L;
    L.add(I.uid, n), L.add(I.replica, intern ? n : 0), L.add(d_type, adopt ? 0 : n), L.add(I.code, n), L.add(I.kind, n);
    L.add(I.held, n), L.add(I.cslot, n), L.add(I.prep, slots), L.add(I.pmin, slots), L.add(I.wp, n), L.add(I.ws, n);
    L.add(I.op, n + 1), L.add(I.os, n + 1), L.add(I.flags, 1), L.add(I.status, n), L.add(I.okind, n), L.add(I.idx, n), L.add(I.slot, n), L.add(I.val, n);
    L.bind(jg::scratch(ctx, ctx->scratch, L.bytes() + 256));
    I.n = n, I.pmask = slots - 1;
    if (!intern) I.replica = nullptr;

    static const bool tr = std::getenv("JANUS_TRACE_ADOPT") != nullptr;
    Trace t{tr, st};
    t.stamp("");
    if (!adopt) {
        JG_HIP(hipMemcpyAsync(I.uid, c.uid, n * sizeof(jg_guid), hipMemcpyHostToDevice, st));
        JG_HIP(hipMemcpyAsync(d_type, c.type, n, hipMemcpyHostToDevice, st));
    }
    if (intern) JG_HIP(hipMemcpyAsync(I.replica, c.replica, n * sizeof(jg_guid), hipMemcpyHostToDevice, st));
    JG_HIP(hipMemsetAsync(I.prep, 0, slots * 4, st));
    JG_HIP(hipMemsetAsync(I.pmin, 0xFF, slots * 4, st));
    JG_HIP(hipMemsetAsync(I.flags, 0, 8, st));
    t.stamp("upload");
    const unsigned g = jg::blocks_for(n, kLanes);
    const DevUids own{nd.tab, nd.mask};
    if (adopt) hipLaunchKernelGGL(k_journal_uids, dim3(g), dim3(kLanes), 0, st, I, c.ks->jglo.as<ull>(), c.ks->jghi.as<ull>(), c.from);
    hipLaunchKernelGGL(k_resolve, dim3(g), dim3(kLanes), 0, st, I, adopt ? (const uint8_t*)nullptr : d_type,
                       adopt ? c.ks->jstatus.as<uint8_t>() : (const uint8_t*)nullptr, c.from, prosp, own);
    t.stamp("k_resolve");
    hipLaunchKernelGGL(k_rank, dim3(g), dim3(kLanes), 0, st, I);
    jgt::excl_scan(ctx, ctx->scratch2, I.wp, I.op, n);
    jgt::excl_scan(ctx, ctx->scratch2, I.ws, I.os, n);
    t.stamp("k_rank + scans");
    const uint32_t has = (nd.pnc ? 1u : 0u) | (nd.orset ? 2u : 0u);
    hipLaunchKernelGGL(k_assign, dim3(g), dim3(kLanes), 0, st, I, nd.next_row, nd.next_set, has, reinterpret_cast<const jg_guid*>(T.cols), T.ncols, T.R,
                       nd.pnc ? nd.pnc->n_keys : 0);
    JG_HIP(hipGetLastError());
    t.stamp("k_assign");
    const auto [tp, ts, flags] = jgt::read_totals(ctx, I.op + n, I.os + n, I.flags);

    // the refusals and the store's growth: nothing has been written so far
    JG_REQUIRE(!(flags & kFlagNoPnc), JG_EINVAL, "%s: a PNCounter to create but the node has no PN-Counter store", c.fn);
    JG_REQUIRE(!(flags & kFlagNoOrset), JG_EINVAL, "%s: an ORSet to create but the node has no OR-Set store", c.fn);
    JG_REQUIRE(ts == 0 || nd.next_set + ts <= 0x7FFFFFF0ull, JG_ESTATE, "%s: %llu more set ids from %u leave the id range", c.fn, (ull)ts, nd.next_set);
    JG_REQUIRE(!(flags & kFlagRowFull), JG_ESTATE, "%s: a new row's replica finds no free column (the row was interned by hand)", c.fn);
    const uint64_t need = nd.next_row + tp;
    if (tp && need > nd.pnc->n_keys) {
        JG_REQUIRE(need <= c.max_keys, JG_ESTATE, "%s: %llu PN-Counter rows needed, the store holds %llu and may grow to %llu (max_keys)", c.fn, (ull)need,
                   (ull)nd.pnc->n_keys, (ull)c.max_keys);
        JG_REQUIRE(!nd.pnc->wave.is_open(), JG_EINVAL, "jg_pnc_reserve: a wave (jg_pnc_wave_begin) is open on this store");
        jg::pnc_grow(nd.pnc, std::min<uint64_t>(std::max<uint64_t>(need, 2 * nd.pnc->n_keys), c.max_keys), nd.pnc->R);
        if (intern) T = jg::pnc_replica_table(nd.pnc);  // the grown table
    }

    t.stamp("host: totals, refusals, growth");
    hipLaunchKernelGGL(k_commit, dim3(g), dim3(kLanes), 0, st, I, nd.tab, nd.mask, reinterpret_cast<jg_guid*>(T.cols), T.ncols, T.R);
    JG_HIP(hipGetLastError());
    t.stamp("k_commit");
    std::vector<uint32_t> slot(n), val(n);
    std::vector<jg_guid> juid(adopt ? n : 0);
    JG_HIP(hipMemcpyAsync(slot.data(), I.slot, n * 4, hipMemcpyDeviceToHost, st));
    JG_HIP(hipMemcpyAsync(val.data(), I.val, n * 4, hipMemcpyDeviceToHost, st));
    if (adopt) JG_HIP(hipMemcpyAsync(juid.data(), I.uid, n * sizeof(jg_guid), hipMemcpyDeviceToHost, st));
    JG_HIP(hipMemcpyAsync(c.status, I.status, n, hipMemcpyDeviceToHost, st));
    if (c.kind) JG_HIP(hipMemcpyAsync(c.kind, I.okind, n, hipMemcpyDeviceToHost, st));
    if (c.idx) JG_HIP(hipMemcpyAsync(c.idx, I.idx, n * 4, hipMemcpyDeviceToHost, st));
    t.stamp("copies out");
    JG_HIP(hipStreamSynchronize(st));
    jg::node_insert_commit(c.node, n, adopt ? juid.data() : c.uid, slot.data(), val.data());
    t.print(c.fn, n);
}

}  // namespace

extern "C" {

int jg_node_next_idx(jg_node* node, uint32_t* next_row, uint32_t* next_set) {
    return jg::guard([&] {
        JG_REQUIRE(node, JG_EINVAL, "jg_node_next_idx: node is NULL");
        auto lk_ = jg::lock(jg::node_ctx(node));
        jg::node_next_idx(node, next_row, next_set);
    });
}

int jg_node_create_uids(jg_node* node, uint64_t n, const jg_guid* uid, const uint8_t* type, const jg_guid* replica, uint64_t max_keys, uint8_t* status,
                        uint32_t* idx) {
    return jg::guard([&] {
        if (n == 0) return;
        JG_REQUIRE(node && uid && type && status, JG_EINVAL, "jg_node_create_uids: NULL argument");
        JG_REQUIRE(n < 0x7FFFFFF0ull, JG_EINVAL, "jg_node_create_uids: at most 2^31 - 16 entries per call");
        auto lk_ = jg::lock(jg::node_ctx(node));
        for (uint64_t i = 0; i < n; ++i) {
            JG_REQUIRE((uid[i].lo | uid[i].hi) != 0, JG_EINVAL, "jg_node_create_uids: entry %llu is Guid.Empty (the key space itself)", (ull)i);
            JG_REQUIRE(type[i] <= 1, JG_EINVAL, "jg_node_create_uids: entry %llu: type %u (0 PNCounter, 1 ORSet)", (ull)i, type[i]);
        }
        Call c{"jg_node_create_uids", node, n};
        c.uid = uid, c.type = type, c.replica = replica, c.max_keys = max_keys, c.status = status, c.idx = idx;
        run(c);
    });
}

int jg_node_adopt_keys(jg_node* stable, jg_node* prospective, jg_keyspace* ks, uint64_t from, uint64_t to, const jg_guid* replica, uint64_t max_keys,
                       uint8_t* status, uint8_t* kind, uint32_t* idx) {
    return jg::guard([&] {
        JG_REQUIRE(stable && prospective && ks, JG_EINVAL, "jg_node_adopt_keys: NULL argument");
        auto lk_ = jg::lock(ks);
        JG_REQUIRE(jg::node_ctx(stable) == ks->ctx && jg::node_ctx(prospective) == ks->ctx, JG_EINVAL,
                   "jg_node_adopt_keys: the key space and the nodes belong to different contexts");
        JG_REQUIRE(from <= to && to <= ks->jn, JG_EINVAL, "jg_node_adopt_keys: records [%llu, %llu) of a journal of %llu", (ull)from, (ull)to, (ull)ks->jn);
        const uint64_t n = to - from;
        if (n == 0) return;
        JG_REQUIRE(status, JG_EINVAL, "jg_node_adopt_keys: status is NULL");
        JG_REQUIRE(n < 0x7FFFFFF0ull, JG_EINVAL, "jg_node_adopt_keys: at most 2^31 - 16 records per call");
        Call c{"jg_node_adopt_keys", stable, n};
        c.prospective = prospective, c.ks = ks, c.from = from, c.replica = replica, c.max_keys = max_keys, c.status = status, c.kind = kind, c.idx = idx;
        run(c);
    });
}

}  // extern "C"
