// update.hip — client writes by key name, resolved on the device: jg_node_update_keys, the same call
// shipping the PN-Counter snapshots SafeCRDT.Update sends next: jg_node_update_keys_encode, and the same
// call shipping every kind's snapshots in one image: jg_node_update_keys_ship, jg_node_shipped, and that
// call with "gp" reads in order among the writes: jg_node_exec_keys.
//
// The reference's "i" / "d" / "a" / "r" / "c" commands (CRDTCommands/PNCounterCommand.cs:42-53, ORSetCommand.cs:43-61) go
// KeySpaceManager.GetKVPair -> SafeCRDT.Update (SafeCRDT.cs:39-47) -> prospectiveState.Update(operationID, args) in
// PNCounterWrapper (PNCounterWrapper.cs:33-48) or ORSetWrapper (ORSetWrapper.cs:30-47).  The tables that chain is made
// of are resident (§9, §11, §12); this file walks them for a batch of commands and applies what resolved:
//
//   k_u_resolve  one lane per command: FNV-1a of the key -> dict_find in the key space's dictionary (tpset_dict.hpp)
//                -> uid_find in the node's uid table (uid_table.hpp) -> (type, row | set), the chain of k_q_resolve,
//                then the two wrappers' status rules.  It writes status, kind, idx and guid, and each wave appends its
//                resolved PN-Counter ops (row, amount, P | N) to one list with one ballot and one atomic
//                (wave_append.hpp).  It reads only: the element table is not touched and no store is written.
//   OR-Set side  the set ids have to reach the host (the Clear epochs and the record walk of apply_ops_names are host
//                work, §11): one D2H of idx | status | kind, the OR-Set commands compacted in batch order, the body of
//                jg_orset_apply_ops_names over them, results scattered back by command index.  It can refuse (a set out
//                of ids, an allocation) and runs before any PN-Counter cell is written.  A node without an OR-Set store
//                skips the round trip; a batch without an OR-Set command launches nothing of it.
//   adds         jg_pnc_apply_ops' wrapping atomic adds over the list (pnc.hip k_add_list), its length read from device
//                memory: a fixed grid, no count on the host.  They cannot refuse once launched.
//
//   snapshots    (jg_node_update_keys_encode only) the resolve also writes (row | none, amount, P | N) per command index:
//                batch order is what a per-command prefix needs, and the appended list has none across waves.
//                pnc_encode.hip plans them (prefixes per row, the survivors of snap == 2, the encode list, its length
//                pass) before the OR-Set side, so the size check refuses before anything is written, and writes them
//                behind it and in front of the adds: both passes read the rows as they stood before the call.
//
//   every kind   (jg_node_update_keys_ship only) the OR-Set commands' survivors are decided on the device like the
//                PN-Counter commands' (snap_survivors.hpp), the host splits them into rounds around the Clears that follow
//                a shipping command, each round is applied and its shipping commands encoded into a region of its own
//                (orset_encode.hip's two phases), and ship_move.hpp's mover merges the regions and the PN-Counter list
//                into one image in command order, which is hashed, copied out once (or held on the node) and followed
//                by the adds.
//
//   reads        (jg_node_exec_keys only; PNCounterCommand.cs:27-41, ORSetCommand.cs:28-42 between the writes of
//                PNCWorkload.cs:44-59 / ORSetWorkload.cs:66-138) k_x_resolve is the same chain with the command kind: a read
//                gets k_q_resolve's statuses, a resolved PN-Counter read enters the per-command arrays on its row with
//                amount 0 and snap 0, so §14's per-row prefixes give it exactly the writes before it and it ships nothing,
//                and each wave appends it to a read list (one ballot, one atomic).  pnc.hip's k_values_at answers the list
//                in front of the adds: Get's checked sums over the row as it stood, with the cell at `col` moved by the
//                prefix.  A resolved OR-Set read rides with the OR-Set commands as the internal op 4 (Contains): Remove's
//                name resolution and membership test in apply_ops' walk, no record, no ord, no round.
//
// The resolve is a dependent chain of random lines: the kernel waits on memory, uses no LDS and few registers, so
// occupancy is what hides the latency.  Nothing is published inside a launch: the kernel boundaries publish the list
// and its count.
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "launch.hpp"
#include "orset_names.hpp"
#include "ship_move.hpp"
#include "tpset_dict.hpp"
#include "uid_table.hpp"
#include "wave_append.hpp"

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kNever = JG_NULL_ELEM - 1;  // "never allocated": the id no record carries (orset_names.hip)
constexpr uint32_t kNoIdx = 0xFFFFFFFFu;       // idx of a command that applied nothing
using ull = unsigned long long;

struct UIn {  // the staged batch
    const ull* koff;
    const long long* amount;  // NULL: no command carries an integer
    const uint8_t *kbytes, *op, *flag;
    const uint8_t* snap;  // _encode only, NULL: 1 for every command
};
struct UOut {
    uint8_t *status, *kind;
    uint32_t* idx;
    jg_guid* guid;
    uint32_t* prow;  // resolved PN-Counter ops: row, amount, 0 = P | 1 = N
    long long* pamt;
    uint8_t* pisn;
    ull* count;  // their number (zeroed before the launch)
    // ORDERED only, one entry per command index: the row (none_row for a command that applies no PN-Counter op), the
    // amount (0 for those), 0 = P | 1 = N
    uint32_t* erow;
    long long* eamt;
    uint8_t* eisn;
};

// jg_node_exec_keys only: which commands are reads, and what the resolve writes for them
struct URd {
    const uint8_t* cmd;  // 0 = write | 1 = read
    long long* value;    // [n] zeroed here; the reads' answers land in it
    uint8_t* ovf;        // [n] zeroed here; k_values_at's overflow byte by command index
    uint32_t *rrow, *rat;  // resolved PN-Counter reads: row, command index
    ull* rcount;         // their number (zeroed before the launch)
};

// READS: a command with cmd 1 is a read.  It gets jg_node_query_keys' statuses; a resolved PN-Counter read enters the
// per-command arrays on its row with amount 0 (so its prefix is the writes before it) and the read list, not the add
// list; a resolved OR-Set read is marked OK for the OR-Set side like a write.
template <bool ORDERED, bool READS>
__device__ __forceinline__ void u_resolve(const jgt::Store& S, const jgt::Dict& D, const jg::DevUids& U, uint64_t pnc_rows, bool has_orset, const UIn& in,
                                          uint64_t n, const UOut& o, const URd& rd) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    bool is_p = false, is_r = false;
    uint32_t row = 0;
    long long amt = 0;
    uint8_t isn = 0;
    if (i < n) {
        uint8_t st = JG_U_NO_KEY, kd = 255;
        uint32_t ix = kNoIdx;
        ull glo = 0, ghi = 0;
        const uint8_t* k = in.kbytes + in.koff[i];
        const uint32_t klen = (uint32_t)(in.koff[i + 1] - in.koff[i]);
        const uint32_t d = jgt::dict_find(S, D, jgt::key_hash(k, klen, S.salt), k, klen);
        if (d != jgt::kNone) {
            glo = D.glo[d], ghi = D.ghi[d];
            const uint32_t v = (glo | ghi) != 0 ? jg::uid_find(U, glo, ghi) : jg::kNoSlot;
            const uint32_t op = in.op[i], flag = in.flag[i];
            if (READS && rd.cmd[i]) {  // JG_Q_* (query.hip k_q_resolve's rules)
                if (v == jg::kNoSlot) {
                    st = JG_Q_NO_CRDT;
                } else if (!(v & jg::kOrSetBit)) {
                    kd = 0;
                    is_r = v < pnc_rows;
                    st = is_r ? JG_Q_OK : JG_Q_NO_CRDT;
                    if (is_r) ix = row = v;
                } else {
                    kd = 1;
                    if (!has_orset) st = JG_Q_NO_CRDT;
                    else if (flag == 0) st = JG_Q_NO_ARG;
                    else st = JG_Q_OK, ix = v & ~jg::kOrSetBit;
                }
            } else if (v == jg::kNoSlot) {
                st = JG_U_NO_CRDT;
            } else if (!(v & jg::kOrSetBit)) {
                kd = 0;
                if (v >= pnc_rows) st = JG_U_NO_CRDT;  // jg_node_register checked the row and stores never shrink
                else if (flag != 3) st = JG_U_BAD_ARG;  // (int)args[0] comes before the switch
                else if (op != 1 && op != 2) st = JG_U_BAD_OP;
                else {
                    st = JG_U_OK;
                    is_p = true;
                    ix = row = v;
                    amt = in.amount[i];
                    isn = op == 2;
                }
            } else {
                kd = 1;
                if (!has_orset) st = JG_U_NO_CRDT;
                else if (op < 1 || op > 3) st = JG_U_BAD_OP;  // the switch comes before args[0]
                else if (op != 3 && flag != 1 && flag != 2) st = JG_U_BAD_ARG;
                else {
                    st = JG_U_OK;
                    ix = v & ~jg::kOrSetBit;
                }
            }
        }
        o.status[i] = st;
        o.kind[i] = kd;
        o.idx[i] = ix;
        if (o.guid) o.guid[i] = jg_guid{glo, ghi};
        if constexpr (ORDERED) o.erow[i] = is_p || is_r ? row : (uint32_t)pnc_rows, o.eamt[i] = amt, o.eisn[i] = isn;
        if constexpr (READS) rd.value[i] = 0, rd.ovf[i] = 0;
    }
    const ull sp = jg::wave_append(is_p, o.count);
    if (is_p) o.prow[sp] = row, o.pamt[sp] = amt, o.pisn[sp] = isn;
    if constexpr (READS) {
        const ull sr = jg::wave_append(is_r, rd.rcount);
        if (is_r) rd.rrow[sr] = row, rd.rat[sr] = (uint32_t)i;
    }
}

template <bool ORDERED>
__global__ __launch_bounds__(kBlock) void k_u_resolve(jgt::Store S, jgt::Dict D, jg::DevUids U, uint64_t pnc_rows, bool has_orset, UIn in, uint64_t n,
                                                      UOut o) {
    u_resolve<ORDERED, false>(S, D, U, pnc_rows, has_orset, in, n, o, URd{});
}

// jg_node_exec_keys' resolve: the same chain with the reads among the writes
__global__ __launch_bounds__(kBlock) void k_x_resolve(jgt::Store S, jgt::Dict D, jg::DevUids U, uint64_t pnc_rows, bool has_orset, UIn in, uint64_t n,
                                                      UOut o, URd rd) {
    u_resolve<true, true>(S, D, U, pnc_rows, has_orset, in, n, o, rd);
}

void check_offsets(const char* what, uint64_t n, const uint64_t* off) {
    JG_REQUIRE(off[0] == 0, JG_EINVAL, "jg_node_update_keys: %s_off[0] must be 0", what);
    for (uint64_t i = 0; i < n; ++i)
        JG_REQUIRE(off[i] <= off[i + 1] && off[i + 1] - off[i] < 0x7FFFFFFFull, JG_EINVAL, "jg_node_update_keys: %s offsets decrease at %llu", what,
                   (ull)i);
    JG_REQUIRE(off[n] < (1ull << 40), JG_EINVAL, "jg_node_update_keys: batch too large");
}

// What every entry point of this file refuses from the arguments alone (n > 0), and how many writes carry each flag.
// cmd (jg_node_exec_keys; NULL: every command is a write) marks the reads: a read may carry no integer, needs no op, no
// amount and no tag, and a batch of reads only may leave op NULL.
struct FlagCounts { uint64_t n[4]; };
FlagCounts check_batch(const jg_node* node, const jg_keyspace* ks, uint64_t n, const uint64_t* key_off, const uint8_t* key_bytes, const uint8_t* op,
                       const uint8_t* arg_flag, const int64_t* amount, const uint64_t* elem_off, const uint8_t* elem_bytes, const uint64_t* tag_lo,
                       const uint64_t* tag_hi, const uint8_t* status, const uint8_t* result, const uint8_t* cmd = nullptr) {
    JG_REQUIRE(node && ks && (op || cmd) && arg_flag && status && result, JG_EINVAL, "jg_node_update_keys: NULL argument");
    JG_REQUIRE(jg::node_ctx(node) == ks->ctx, JG_EINVAL, "jg_node_update_keys: the key space and the node belong to different contexts");
    JG_REQUIRE(n < 0x7FFFFFF0ull, JG_EINVAL, "jg_node_update_keys: at most 2^31 commands per call");
    JG_REQUIRE(key_off, JG_EINVAL, "jg_node_update_keys: key_off is NULL");
    check_offsets("key", n, key_off);
    JG_REQUIRE(key_off[n] == 0 || key_bytes, JG_EINVAL, "jg_node_update_keys: key_bytes is NULL");
    if (elem_off) check_offsets("elem", n, elem_off);
    FlagCounts c{{0, 0, 0, 0}};
    uint64_t n_str = 0, n_write = 0;
    for (uint64_t i = 0; i < n; ++i) {
        JG_REQUIRE(arg_flag[i] <= 3, JG_EINVAL, "jg_node_update_keys: arg_flag[%llu] = %u (0 none, 1 string, 2 null, 3 integer)", (ull)i, arg_flag[i]);
        n_str += arg_flag[i] == 1;
        if (cmd) {
            JG_REQUIRE(cmd[i] <= 1, JG_EINVAL, "jg_node_exec_keys: cmd[%llu] = %u (0 write, 1 read)", (ull)i, cmd[i]);
            JG_REQUIRE(!cmd[i] || arg_flag[i] != 3, JG_EINVAL, "jg_node_exec_keys: read %llu carries an integer", (ull)i);
            if (cmd[i]) continue;
        }
        ++n_write;
        ++c.n[arg_flag[i]];
    }
    JG_REQUIRE(n_write == 0 || op, JG_EINVAL, "jg_node_update_keys: NULL argument");
    JG_REQUIRE(c.n[3] == 0 || amount, JG_EINVAL, "jg_node_update_keys: a command carries an integer and amount is NULL");
    JG_REQUIRE(n_str == 0 || (elem_off && elem_bytes), JG_EINVAL, "jg_node_update_keys: a command carries a string and elem_off or elem_bytes is NULL");
    JG_REQUIRE(c.n[1] + c.n[2] == 0 || (tag_lo && tag_hi), JG_EINVAL, "jg_node_update_keys: a command carries an element and tag_lo or tag_hi is NULL");
    return c;
}

// what jg_node_update_keys_encode adds to jg_node_update_keys' arguments
struct Enc {
    const uint8_t* snap;
    uint64_t* snap_off;
    uint8_t* out;
    uint64_t cap;
    uint8_t* sha;
};

// Both entry points (enc NULL: jg_node_update_keys, which launches and answers as it did before the other existed).
int update_keys(jg_node* node, jg_keyspace* ks, uint64_t n, const uint64_t* key_off, const uint8_t* key_bytes, const uint8_t* op,
                const uint8_t* arg_flag, const int64_t* amount, const uint64_t* elem_off, const uint8_t* elem_bytes, const uint64_t* tag_lo,
                const uint64_t* tag_hi, uint32_t col, uint8_t* status, uint8_t* result, uint8_t* kind, uint32_t* idx, uint32_t* elem, jg_guid* guid,
                uint64_t* add_lim, uint64_t* rem_lim, const Enc* enc) {
    return jg::guard([&] {
        auto lk_ = jg::lock(ks);  // calls on one context are serialised (shared scratch, stream)
        JG_REQUIRE(!enc || enc->snap_off, JG_EINVAL, "jg_node_update_keys_encode: snap_off is NULL");
        if (n == 0) {
            if (enc) enc->snap_off[0] = 0;
            return;
        }
        // every refusal below is decided from the arguments: nothing has been copied or written yet
        const FlagCounts n_flag = check_batch(node, ks, n, key_off, key_bytes, op, arg_flag, amount, elem_off, elem_bytes, tag_lo, tag_hi, status, result);
        JG_REQUIRE(!add_lim == !rem_lim, JG_EINVAL, "jg_node_update_keys: add_lim and rem_lim go together");
        if (enc) {  // a snapshot needs an applied PN-Counter command, which needs an integer: decided from the arguments
            bool may_ship = false;
            for (uint64_t i = 0; i < n; ++i) {
                JG_REQUIRE(!enc->snap || enc->snap[i] <= 2, JG_EINVAL, "jg_node_update_keys_encode: snap[%llu] = %u (0 none, 1 this command's, 2 the latest)",
                           (ull)i, enc->snap[i]);
                may_ship |= arg_flag[i] == 3 && (!enc->snap || enc->snap[i] != 0);
            }
            JG_REQUIRE(!may_ship || enc->out, JG_EINVAL, "jg_node_update_keys_encode: a command may ship a snapshot and out is NULL");
        }
        jg_ctx* ctx = ks->ctx;
        jg::ensure_device(ctx);
        const jg::NodeRef nd = jg::node_query_ref(node, "jg_node_update_keys");  // pending registrations to the device
        JG_REQUIRE(!nd.pnc || col < nd.pnc->R, JG_EINVAL, "jg_node_update_keys: column %u outside the PN-Counter store's %u", col,
                   nd.pnc ? nd.pnc->R : 0);
        jg::require_writable(nd.pnc, "jg_node_update_keys");
        jg::require_writable(nd.orset, "jg_node_update_keys");
        JG_REQUIRE(!nd.orset || !jg::orset_wave_open(nd.orset), JG_EINVAL, "jg_node_update_keys: a wave is open on the OR-Set store");

        // keys, ops, flags and amounts in one staging copy: koff | amount | key bytes | op | flag.  The elements stay on the
        // host: only the OR-Set side reads them, compacted.
        const uint64_t kb = key_off[n];
        const bool ints = n_flag.n[3] != 0;
        UIn in{};
        UOut o{};
        jg::Layout L;
        L.add(in.koff, n + 1, 8), L.add(in.amount, ints ? n : 0, 8), L.add(in.kbytes, kb, 8), L.add(in.op, n, 1), L.add(in.flag, n, 1);
        const bool snaps = enc && enc->snap;
        L.add(in.snap, snaps ? n : 0, 1);
        const size_t stage = L.skip(0, 8);
        std::vector<uint8_t> h(stage);
        L.bind(h.data());  // the host image first: the same offsets as on the device
        std::memcpy(h.data(), key_off, (n + 1) * 8);
        if (ints) std::memcpy(const_cast<long long*>(in.amount), amount, n * 8);
        if (kb) std::memcpy(const_cast<uint8_t*>(in.kbytes), key_bytes, kb);
        std::memcpy(const_cast<uint8_t*>(in.op), op, n);
        std::memcpy(const_cast<uint8_t*>(in.flag), arg_flag, n);
        if (snaps) std::memcpy(const_cast<uint8_t*>(in.snap), enc->snap, n);
        // behind it (16 bytes on): count | guid | pamt | prow | idx | status | kind | pisn; idx, status and kind are one
        // stretch of 6 n bytes (one copy out)
        L.skip(16);
        L.add(o.count, 1, 8), L.add(o.guid, guid ? n : 0, 8), L.add(o.pamt, n, 8), L.add(o.prow, n, 4);
        L.add(o.idx, n, 4), L.add(o.status, n, 1), L.add(o.kind, n, 1), L.add(o.pisn, n, 1);
        // _encode: the ops by command index and the snapshots' arrays, which outlive the OR-Set side like the rest
        const bool plan = enc && nd.pnc;
        jg::PncSnap sn{};
        L.add(o.eamt, enc ? n : 0, 8), L.add(o.erow, enc ? n : 0, 4), L.add(o.eisn, enc ? n : 0, 1);
        if (plan) sn.carve(L, n);
        auto* d = static_cast<uint8_t*>(jg::scratch(ctx, ctx->scratch_u, L.bytes() + 64));
        L.bind(d);
        if (!ints) in.amount = nullptr;
        if (!snaps) in.snap = nullptr;
        sn.row = o.erow, sn.amount = o.eamt, sn.is_n = o.eisn, sn.snap = in.snap;
        if (!guid) o.guid = nullptr;

        // JANUS_TRACE_UPDATE (as JANUS_TRACE_QUERY): the upload, the launches and the copies out by hipEvents
        static const bool tr = std::getenv("JANUS_TRACE_UPDATE") != nullptr;
        hipEvent_t ev[8] = {}, sev[5] = {};  // sev: the snapshot steps' own (pnc_snap_*_locked)
        auto stamp = [&](int k) {
            if (!tr) return;
            JG_HIP(hipEventCreate(&ev[k]));
            JG_HIP(hipEventRecord(ev[k], ctx->stream));
        };
        stamp(0);
        JG_HIP(hipMemcpyAsync(d, h.data(), stage, hipMemcpyHostToDevice, ctx->stream));
        stamp(1);
        JG_HIP(hipMemsetAsync(o.count, 0, 8, ctx->stream));
        const auto resolve = enc ? k_u_resolve<true> : k_u_resolve<false>;
        hipLaunchKernelGGL(resolve, dim3(jg::blocks_for(n)), dim3(kBlock), 0, ctx->stream, ks->set->view(), ks->dict(), nd.uids,
                           nd.pnc ? nd.pnc->n_keys : 0, nd.orset != nullptr, in, n, o);
        JG_HIP(hipGetLastError());
        stamp(2);

        // idx | status | kind on the host: before the OR-Set side where the node has one, else with the other copies out
        std::vector<uint8_t> hres(n * 6);
        const auto* h_idx = reinterpret_cast<const uint32_t*>(hres.data());
        const uint8_t *h_status = hres.data() + n * 4, *h_kind = hres.data() + n * 5;
        std::vector<uint8_t> res(n, 0);
        std::vector<uint32_t> el(elem ? n : 0, kNever);
        std::vector<uint64_t> al(add_lim ? n : 0, 0), rl(add_lim ? n : 0, 0);
        double host_ms = 0;
        uint64_t n_o = 0;
        // _encode: the snapshots planned and sized before the OR-Set side writes anything.  A batch past `cap` is refused
        // here with its offsets filled: nothing has been applied.
        std::vector<uint64_t> hoff(enc ? n + 1 : 0, 0);
        uint64_t n_snap = 0;
        if (nd.orset) JG_HIP(hipMemcpyAsync(hres.data(), o.idx, n * 6, hipMemcpyDeviceToHost, ctx->stream));
        if (plan) {
            try {
                if (tr)
                    for (hipEvent_t& e : sev) JG_HIP(hipEventCreate(&e));
                jg::pnc_snap_plan_locked(nd.pnc, sn, n, col, &n_snap, hoff.data(), tr ? sev : nullptr);
            } catch (...) {
                (void)hipStreamSynchronize(ctx->stream);  // the copy into hres above
                throw;
            }
            if (hoff[n] > enc->cap) {
                std::memcpy(enc->snap_off, hoff.data(), (n + 1) * 8);
                jg::fail(JG_ESTATE, "jg_node_update_keys_encode: %llu bytes exceed cap %llu (nothing applied)", (ull)hoff[n], (ull)enc->cap);
            }
        }
        stamp(6);
        if (nd.orset) {
            JG_HIP(hipStreamSynchronize(ctx->stream));
            const double t0 = jg::now_us();
            std::vector<uint32_t> at;  // the OR-Set commands, in batch order
            for (uint64_t i = 0; i < n; ++i)
                if (h_status[i] == JG_U_OK && h_kind[i] == 1) at.push_back((uint32_t)i);
            n_o = at.size();
            if (n_o) {
                std::vector<uint32_t> oset(n_o), oel(n_o);
                std::vector<uint8_t> oop(n_o), onull(n_o), ores(n_o), obytes;
                std::vector<uint64_t> ooff(n_o + 1, 0), olo(n_o), ohi(n_o), oal(add_lim ? n_o : 0), orl(add_lim ? n_o : 0);
                for (uint64_t k = 0; k < n_o; ++k) {
                    const uint32_t i = at[k];
                    const bool str = op[i] != 3 && arg_flag[i] == 1;  // a Clear ignores its argument
                    oset[k] = h_idx[i], oop[k] = op[i], onull[k] = op[i] != 3 && arg_flag[i] == 2;
                    olo[k] = tag_lo ? tag_lo[i] : 0, ohi[k] = tag_hi ? tag_hi[i] : 0;  // NULL: the batch's OR-Set commands are all Clears
                    if (str) obytes.insert(obytes.end(), elem_bytes + elem_off[i], elem_bytes + elem_off[i + 1]);
                    ooff[k + 1] = obytes.size();
                }
                if (obytes.empty()) obytes.push_back(0);
                // all or nothing: a refusal here has written no PN-Counter cell, and apply_ops_names leaves its own store,
                // the element table and the names log as they were
                jg::orset_apply_ops_names_locked(nd.orset, n_o, oset.data(), oop.data(), ooff.data(), obytes.data(), onull.data(), olo.data(),
                                                 ohi.data(), ores.data(), oel.data(), add_lim ? oal.data() : nullptr, add_lim ? orl.data() : nullptr);
                for (uint64_t k = 0; k < n_o; ++k) {
                    const uint32_t i = at[k];
                    res[i] = ores[k];
                    if (elem) el[i] = oel[k];
                    if (add_lim) al[i] = oal[k], rl[i] = orl[k];
                }
            }
            host_ms = (jg::now_us() - t0) * 1e-3;
        }
        stamp(3);
        // the write pass reads the rows as they stand, the adds land behind it
        if (plan) jg::pnc_snap_write_locked(nd.pnc, sn, n, n_snap, hoff[n], col, enc->out, enc->sha, tr ? sev : nullptr);
        stamp(7);
        if (nd.pnc) jg::pnc_add_list_device(nd.pnc, o.prow, o.pamt, o.pisn, o.count, n, col);
        stamp(4);
        if (!nd.orset) JG_HIP(hipMemcpyAsync(hres.data(), o.idx, n * 6, hipMemcpyDeviceToHost, ctx->stream));
        if (guid) JG_HIP(hipMemcpyAsync(guid, o.guid, n * sizeof(jg_guid), hipMemcpyDeviceToHost, ctx->stream));
        stamp(5);
        JG_HIP(hipStreamSynchronize(ctx->stream));
        for (uint64_t i = 0; i < n; ++i)
            if (h_status[i] == JG_U_OK && h_kind[i] == 0) res[i] = 1;
        std::memcpy(status, h_status, n);
        std::memcpy(result, res.data(), n);
        if (kind) std::memcpy(kind, h_kind, n);
        if (idx) std::memcpy(idx, h_idx, n * 4);
        if (elem) std::memcpy(elem, el.data(), n * 4);
        if (add_lim) std::memcpy(add_lim, al.data(), n * 8), std::memcpy(rem_lim, rl.data(), n * 8);
        if (enc) {
            std::memcpy(enc->snap_off, hoff.data(), (n + 1) * 8);
            if (!plan && enc->sha) std::memset(enc->sha, 0, n * 32);
        }
        if (tr) {
            float up = 0, run = 0, add = 0, down = 0;
            JG_HIP(hipEventElapsedTime(&up, ev[0], ev[1]));
            JG_HIP(hipEventElapsedTime(&run, ev[1], ev[2]));
            JG_HIP(hipEventElapsedTime(&add, ev[7], ev[4]));
            JG_HIP(hipEventElapsedTime(&down, ev[4], ev[5]));
            std::fprintf(stderr, "update_keys(%llu commands, %llu bytes up, %llu bytes down): upload %.3f ms, resolve launch %.3f ms, "
                         "PN-Counter adds %.3f ms, copies out %.3f ms; OR-Set side (%llu commands, after a copy of 6 bytes per command) %.3f ms\n",
                         (ull)n, (ull)stage, (ull)(n * (6 + (guid ? 16 : 0))), up, run, add, down, (ull)n_o, host_ms);
            if (plan) {  // the second step waits for the host in front of it (the list's length): that gap is its own
                float pre = 0, len = 0, wr = 0, sha = 0, cp = 0;
                JG_HIP(hipEventElapsedTime(&pre, ev[2], sev[0]));
                JG_HIP(hipEventElapsedTime(&len, sev[0], sev[1]));
                JG_HIP(hipEventElapsedTime(&wr, ev[3], sev[2]));
                JG_HIP(hipEventElapsedTime(&sha, sev[2], sev[3]));
                JG_HIP(hipEventElapsedTime(&cp, sev[3], sev[4]));
                std::fprintf(stderr, "update_keys_encode(%llu snapshots, %llu bytes): prefixes, survivors and list %.3f ms, length pass and offsets "
                             "(behind a host wait) %.3f ms, write pass %.3f ms, hashes %.3f ms, copy of the bytes %.3f ms\n", (ull)n_snap, (ull)hoff[n],
                             pre, len, wr, sha, cp);
                for (hipEvent_t e : sev) (void)hipEventDestroy(e);
            }
            for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        }
    });
}

// ---- jg_node_update_keys_ship: every snapshot of the batch, OR-Set keys included ---------------------
// command i's object among the OR-Set sets: its set id, or none_obj for every command that is not an applied OR-Set command
__global__ __launch_bounds__(kBlock) void k_u_ship_obj(const uint8_t* __restrict__ status, const uint8_t* __restrict__ kind,
                                                       const uint32_t* __restrict__ idx, uint64_t n, uint32_t none_obj, uint32_t* __restrict__ obj) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) obj[i] = status[i] == JG_U_OK && kind[i] == 1 ? idx[i] : none_obj;
}

// jg_node_exec_keys' two arguments more; NULL: jg_node_update_keys_ship, which launches and answers as
// it did before the other existed
struct Exec {
    const uint8_t* cmd;  // 0 = write | 1 = read
    int64_t* value;      // the reads' answers, 0 for every other command
};

int update_keys_ship(jg_node* node, jg_keyspace* ks, uint64_t n, const uint64_t* key_off, const uint8_t* key_bytes, const uint8_t* op,
                     const uint8_t* arg_flag, const int64_t* amount, const uint64_t* elem_off, const uint8_t* elem_bytes, const uint64_t* tag_lo,
                     const uint64_t* tag_hi, uint32_t col, const uint8_t* snap, uint8_t* status, uint8_t* result, uint8_t* kind, uint32_t* idx,
                     uint32_t* elem, jg_guid* guid, uint64_t* snap_off, uint64_t* n_bytes, uint8_t* out, uint64_t cap, uint8_t* sha, uint32_t* n_rounds,
                     const Exec* ex = nullptr) {
    return jg::guard([&] {
        auto lk_ = jg::lock(ks);
        JG_REQUIRE(snap_off && n_bytes, JG_EINVAL, "jg_node_update_keys_ship: snap_off or n_bytes is NULL");
        if (n == 0) {
            snap_off[0] = 0, *n_bytes = 0;
            if (n_rounds) *n_rounds = 0;
            return;
        }
        // every refusal below is decided from the arguments: nothing has been copied or written yet
        JG_REQUIRE(!ex || (ex->cmd && ex->value), JG_EINVAL, "jg_node_exec_keys: cmd or value is NULL");
        const uint8_t* cmd = ex ? ex->cmd : nullptr;
        const FlagCounts n_flag =
            check_batch(node, ks, n, key_off, key_bytes, op, arg_flag, amount, elem_off, elem_bytes, tag_lo, tag_hi, status, result, cmd);
        const auto reads = [&](uint64_t i) { return cmd && cmd[i]; };
        uint64_t n_reads = 0;
        for (uint64_t i = 0; cmd && i < n; ++i) n_reads += cmd[i];
        for (uint64_t i = 0; snap && i < n; ++i)
            JG_REQUIRE(reads(i) || snap[i] <= 2, JG_EINVAL, "jg_node_update_keys_ship: snap[%llu] = %u (0 none, 1 this command's, 2 the latest)", (ull)i,
                       snap[i]);
        JG_REQUIRE(out || cap == 0, JG_EINVAL, "jg_node_update_keys_ship: out is NULL and cap is not 0");
        jg_ctx* ctx = ks->ctx;
        jg::ensure_device(ctx);
        const jg::NodeRef nd = jg::node_query_ref(node, "jg_node_update_keys_ship");
        JG_REQUIRE(!nd.pnc || col < nd.pnc->R, JG_EINVAL, "jg_node_update_keys_ship: column %u outside the PN-Counter store's %u", col,
                   nd.pnc ? nd.pnc->R : 0);
        jg::require_writable(nd.pnc, "jg_node_update_keys_ship");
        jg::require_writable(nd.orset, "jg_node_update_keys_ship");
        JG_REQUIRE(!nd.orset || !jg::orset_wave_open(nd.orset), JG_EINVAL, "jg_node_update_keys_ship: a wave is open on the OR-Set store");
        jg::ShipState& ship = jg::node_ship(node);

        // the batch as jg_node_update_keys_encode stages it, and behind it what only this call needs: the OR-Set objects,
        // their no-snapshot flags, and the mover's list (source address, merged offset, merged no-snapshot flag)
        const uint64_t kb = key_off[n];
        // with reads the snap bytes are always staged: a read's is 0, so it ships nothing and, in snap_survivors.hpp's
        // rule, never stands for a later snap == 2 command of its object
        const bool ints = n_flag.n[3] != 0, snaps = snap != nullptr || ex, plan = nd.pnc != nullptr;
        UIn in{};
        UOut o{};
        URd rd{};
        jg::Layout L;
        L.add(in.koff, n + 1, 8), L.add(in.amount, ints ? n : 0, 8), L.add(in.kbytes, kb, 8), L.add(in.op, n, 1), L.add(in.flag, n, 1);
        L.add(in.snap, snaps ? n : 0, 1);
        if (ex) L.add(rd.cmd, n, 1);
        const size_t stage = L.skip(0, 8);
        std::vector<uint8_t> h(stage);
        L.bind(h.data());
        std::memcpy(h.data(), key_off, (n + 1) * 8);
        if (ints) std::memcpy(const_cast<long long*>(in.amount), amount, n * 8);
        if (kb) std::memcpy(const_cast<uint8_t*>(in.kbytes), key_bytes, kb);
        if (op) std::memcpy(const_cast<uint8_t*>(in.op), op, n);  // (NULL: a batch of reads, the bytes stay 0)
        std::memcpy(const_cast<uint8_t*>(in.flag), arg_flag, n);
        if (snap) std::memcpy(const_cast<uint8_t*>(in.snap), snap, n);
        if (ex) {
            auto* hs = const_cast<uint8_t*>(in.snap);
            std::memcpy(const_cast<uint8_t*>(rd.cmd), cmd, n);
            for (uint64_t i = 0; i < n; ++i) hs[i] = cmd[i] ? 0 : snap ? snap[i] : 1;
        }
        L.skip(16);
        L.add(o.count, 1, 8), L.add(o.guid, guid ? n : 0, 8), L.add(o.pamt, n, 8), L.add(o.prow, n, 4);
        L.add(o.idx, n, 4), L.add(o.status, n, 1), L.add(o.kind, n, 1), L.add(o.pisn, n, 1);
        jg::PncSnap sn{};
        L.add(o.eamt, n, 8), L.add(o.erow, n, 4), L.add(o.eisn, n, 1);
        if (plan) sn.carve(L, n, ex != nullptr);
        // the reads' answers and, for the PN-Counter reads, their list: value | rcount | rrow | rat | ovf
        if (ex) L.add(rd.value, n, 8), L.add(rd.rcount, 1, 8), L.add(rd.rrow, n, 4), L.add(rd.rat, n, 4), L.add(rd.ovf, n, 1);
        uint32_t* oobj;
        uint8_t *onone, *mlist;
        ull *msrc, *moff;
        uint8_t* mnone;
        L.add(oobj, n, 4), L.add(onone, n, 1);
        const size_t mlist_at = L.add(msrc, n, 16), mlist_bytes = n * 8 + (n + 1) * 8 + n;  // one stretch, one copy up
        L.add(moff, n + 1, 8), L.add(mnone, n, 1);
        auto* d = static_cast<uint8_t*>(jg::scratch(ctx, ctx->scratch_u, L.bytes() + 64));
        L.bind(d);
        mlist = d + mlist_at;
        if (!ints) in.amount = nullptr;
        if (!snaps) in.snap = nullptr;
        sn.row = o.erow, sn.amount = o.eamt, sn.is_n = o.eisn, sn.snap = in.snap;
        if (!guid) o.guid = nullptr;

        // JANUS_TRACE_UPDATE: the steps by the host's clock (each ends at a wait on the stream) and, by hipEvents, the
        // mover, the hashes and the copy
        static const bool tr = std::getenv("JANUS_TRACE_UPDATE") != nullptr;
        double t_mark = jg::now_us();
        const auto lap = [&] {
            const double t = jg::now_us(), ms = (t - t_mark) * 1e-3;
            t_mark = t;
            return ms;
        };
        hipEvent_t ev[4] = {};
        const auto stamp = [&](int k) {
            if (!tr) return;
            JG_HIP(hipEventCreate(&ev[k]));
            JG_HIP(hipEventRecord(ev[k], ctx->stream));
        };

        JG_HIP(hipMemcpyAsync(d, h.data(), stage, hipMemcpyHostToDevice, ctx->stream));
        JG_HIP(hipMemsetAsync(o.count, 0, 8, ctx->stream));
        if (ex) {
            JG_HIP(hipMemsetAsync(rd.rcount, 0, 8, ctx->stream));
            hipLaunchKernelGGL(k_x_resolve, dim3(jg::blocks_for(n)), dim3(kBlock), 0, ctx->stream, ks->set->view(), ks->dict(), nd.uids,
                               nd.pnc ? nd.pnc->n_keys : 0, nd.orset != nullptr, in, n, o, rd);
        } else {
            hipLaunchKernelGGL(k_u_resolve<true>, dim3(jg::blocks_for(n)), dim3(kBlock), 0, ctx->stream, ks->set->view(), ks->dict(), nd.uids,
                               nd.pnc ? nd.pnc->n_keys : 0, nd.orset != nullptr, in, n, o);
        }
        JG_HIP(hipGetLastError());
        std::vector<uint8_t> hres(n * 6), hnone(n, 1);
        const auto* h_idx = reinterpret_cast<const uint32_t*>(hres.data());
        const uint8_t *h_status = hres.data() + n * 4, *h_kind = hres.data() + n * 5;
        JG_HIP(hipMemcpyAsync(hres.data(), o.idx, n * 6, hipMemcpyDeviceToHost, ctx->stream));
        double ms_resolve = 0, ms_surv = 0, ms_pnc = 0, ms_dry = 0, ms_apply = 0, ms_enc = 0;
        if (tr) {
                JG_HIP(hipStreamSynchronize(ctx->stream));
                ms_resolve = lap();
            }
        // the survivors of both kinds on the device (snap_survivors.hpp): the OR-Set commands by set id here, the PN-Counter
        // commands by row in the plan below.  The OR-Set flags come down with idx | status | kind.
        try {
            if (nd.orset) {
                const uint32_t none_obj = nd.max_set + 1;
                hipLaunchKernelGGL(k_u_ship_obj, dim3(jg::blocks_for(n)), dim3(kBlock), 0, ctx->stream, o.status, o.kind, o.idx, n, none_obj, oobj);
                JG_HIP(hipGetLastError());
                jg::snap_survivors_locked(ctx, oobj, n, none_obj, in.snap, onone);
                JG_HIP(hipMemcpyAsync(hnone.data(), onone, n, hipMemcpyDeviceToHost, ctx->stream));
            }
            if (tr) {
                JG_HIP(hipStreamSynchronize(ctx->stream));
                ms_surv = lap();
            }
        } catch (...) {
            (void)hipStreamSynchronize(ctx->stream);  // the copies into hres and hnone
            throw;
        }
        // the PN-Counter snapshots planned and sized (§14's step 1; it reads only and waits on the stream)
        std::vector<uint64_t> hoff_p(n + 1, 0);
        uint64_t n_snap = 0;
        try {
            if (plan) jg::pnc_snap_plan_locked(nd.pnc, sn, n, col, &n_snap, hoff_p.data(), nullptr);
        } catch (...) {
            (void)hipStreamSynchronize(ctx->stream);
            throw;
        }
        JG_HIP(hipStreamSynchronize(ctx->stream));
        if (tr) ms_pnc = lap();

        // the OR-Set commands in batch order, who of them ships, and each one's round: per set, a Clear starts a new round
        // iff a shipping command on the set lies between the set's previous Clear (or the batch start) and it
        std::vector<uint32_t> at;
        for (uint64_t i = 0; i < n; ++i)
            if (h_status[i] == JG_U_OK && h_kind[i] == 1) at.push_back((uint32_t)i);
        const uint64_t n_o = nd.orset ? at.size() : 0;
        // a read among them (status and kind say the same for both) runs as the internal op 4, Contains: it takes the round
        // current for its set, opens and cuts none, and is not counted in *n_rounds
        std::vector<uint8_t> eop_v;
        if (ex) {
            eop_v.resize(n);
            for (uint64_t i = 0; i < n; ++i) eop_v[i] = cmd[i] ? 4 : op[i];
        }
        const uint8_t* eop = ex ? eop_v.data() : op;
        std::vector<uint32_t> round(n_o, 0);
        uint32_t rounds = 0;
        uint64_t max_adds = 0;
        std::vector<uint32_t> ship_sets;
        if (n_o) {
            struct PerSet { uint32_t round = 0, adds = 0; bool open = false, ships = false; };  // open: a command shipped since the last Clear
            std::vector<PerSet> per((size_t)nd.max_set + 1);
            for (uint64_t k = 0; k < n_o; ++k) {
                const uint32_t i = at[k];
                PerSet& ps = per[h_idx[i]];
                if (eop[i] == 3 && ps.open) ++ps.round, ps.open = false;
                round[k] = ps.round;
                if (eop[i] != 4) rounds = std::max(rounds, ps.round + 1);
                if (!hnone[i]) {
                    if (!ps.ships) ship_sets.push_back(h_idx[i]);
                    ps.open = ps.ships = true;
                }
                if (eop[i] == 1 && arg_flag[i] == 1) max_adds = std::max<uint64_t>(max_adds, ++ps.adds);
            }
        }
        const uint32_t passes = std::max<uint32_t>(rounds, n_o ? 1 : 0);  // a batch whose OR-Set commands are all reads: one pass, no round
        // refusals that need the stores, still before anything is written: a shipping set with a record whose element id has
        // no name (the encoder's size phase, without limits, over the distinct shipping sets), and a batch of several rounds
        // that could run a set out of element ids in a later round
        std::vector<uint64_t> roff;
        if (!ship_sets.empty()) {
            roff.resize(ship_sets.size() + 1);
            JG_REQUIRE(jg::orset_encode_size_locked(nd.orset, ship_sets.size(), ship_sets.data(), nullptr, nullptr, roff.data()), JG_ESTATE,
                       "jg_node_update_keys_ship: a set that would ship holds a record whose element id has no name in the element table (names not "
                       "synced; nothing applied)");
        }
        if (rounds > 1) {
            jg::ElemTable& T = *jg::orset_elem_table(nd.orset, true);
            if (T.id_bound + max_adds >= kNever) T.tight_id_bound(ctx, ctx->scratch3);
            JG_REQUIRE(T.id_bound + max_adds < kNever, JG_ESTATE,
                       "jg_node_update_keys_ship: a batch of %u rounds could leave a set without element ids (nothing applied)", rounds);
        }
        if (tr) ms_dry = lap();

        // the rounds: apply round r's commands in batch order, then size and write its shipping commands' states at the ord
        // limits the apply returned, into the round's own region.  Round 0's apply can still refuse; nothing is written then.
        std::vector<uint8_t> res(n, 0);
        std::vector<uint32_t> el(elem ? n : 0, kNever);
        std::vector<uint64_t> len(n, 0), src(n, 0);
        std::vector<int64_t> val(ex ? n : 0, 0);
        for (uint32_t r = 0; r < passes; ++r) {
            std::vector<uint32_t> rcmd, oset, oel;
            std::vector<uint8_t> oop, onull, ores, obytes;
            std::vector<uint64_t> ooff{0}, olo, ohi;
            for (uint64_t k = 0; k < n_o; ++k) {
                if (round[k] != r) continue;
                const uint32_t i = at[k];
                rcmd.push_back(i), oset.push_back(h_idx[i]), oop.push_back(eop[i]), onull.push_back(eop[i] != 3 && arg_flag[i] == 2);
                olo.push_back(tag_lo && eop[i] != 4 ? tag_lo[i] : 0), ohi.push_back(tag_hi && eop[i] != 4 ? tag_hi[i] : 0);
                if (eop[i] != 3 && arg_flag[i] == 1) obytes.insert(obytes.end(), elem_bytes + elem_off[i], elem_bytes + elem_off[i + 1]);
                ooff.push_back(obytes.size());
            }
            const uint64_t n_r = rcmd.size();
            if (obytes.empty()) obytes.push_back(0);
            ores.resize(n_r), oel.resize(n_r);
            std::vector<uint64_t> oal(n_r), orl(n_r);
            jg::orset_apply_ops_names_locked(nd.orset, n_r, oset.data(), oop.data(), ooff.data(), obytes.data(), onull.data(), olo.data(), ohi.data(),
                                             ores.data(), oel.data(), oal.data(), orl.data(), ex != nullptr);
            std::vector<uint32_t> scmd, sset;
            std::vector<uint64_t> sal, srl;
            for (uint64_t k = 0; k < n_r; ++k) {
                const uint32_t i = rcmd[k];
                if (reads(i)) val[i] = ores[k];  // Contains' answer; a read's result stays 0
                else res[i] = ores[k];
                if (elem) el[i] = oel[k];
                if (!hnone[i]) scmd.push_back(i), sset.push_back(oset[k]), sal.push_back(oal[k]), srl.push_back(orl[k]);
            }
            if (tr) ms_apply += lap();
            const uint64_t n_s = scmd.size();
            if (n_s) {
                roff.resize(n_s + 1);
                JG_REQUIRE(jg::orset_encode_size_locked(nd.orset, n_s, sset.data(), sal.data(), srl.data(), roff.data()), JG_ESTATE,
                           "jg_node_update_keys_ship: a record names an element id the element table does not hold");
                while (ship.region.size() <= r) ship.region.push_back(std::make_unique<jg::DevBuf>());
                jg::DevBuf& reg = *ship.region[r];
                jg::ensure(reg, roff[n_s] + 64);
                jg::orset_encode_write_locked(nd.orset, reg.as<uint8_t>());
                for (uint64_t k = 0; k < n_s; ++k) len[scmd[k]] = roff[k + 1] - roff[k], src[scmd[k]] = (uint64_t)(uintptr_t)reg.p + roff[k];
            }
            if (tr) {
                JG_HIP(hipStreamSynchronize(ctx->stream));
                ms_enc += lap();
            }
        }
        // the PN-Counter list's bytes (the rows as they stand: the adds land behind the image), then the mover's list
        if (n_snap) {
            const uint8_t* dpnc = jg::pnc_snap_bytes_locked(nd.pnc, sn, n_snap, hoff_p[n], col);
            for (uint64_t i = 0; i < n; ++i)
                if (hoff_p[i + 1] != hoff_p[i]) len[i] = hoff_p[i + 1] - hoff_p[i], src[i] = (uint64_t)(uintptr_t)dpnc + hoff_p[i];
        }
        std::vector<uint8_t> hm(mlist_bytes);
        auto* h_src = reinterpret_cast<uint64_t*>(hm.data());
        auto* h_off = h_src + n;
        uint8_t* h_none = reinterpret_cast<uint8_t*>(h_off + n + 1);
        h_off[0] = 0;
        for (uint64_t i = 0; i < n; ++i) h_src[i] = src[i], h_off[i + 1] = h_off[i] + len[i], h_none[i] = len[i] == 0;
        const uint64_t total = h_off[n];
        stamp(0);
        if (total) {
            ship.held = false;  // the image an earlier call left is overwritten here
            jg::ensure(ship.image, total + 64);
            JG_HIP(hipMemcpyAsync(mlist, hm.data(), mlist_bytes, hipMemcpyHostToDevice, ctx->stream));
            ship_move(ctx->stream, msrc, moff, n, ship.image.as<uint8_t>());
            JG_HIP(hipGetLastError());
        }
        stamp(1);
        if (sha && total) jg::sha256_device(ctx, ship.image.as<uint8_t>(), reinterpret_cast<const uint64_t*>(moff), n, sha, mnone);
        stamp(2);
        const bool fits = total <= cap;
        if (total && fits) JG_HIP(hipMemcpyAsync(out, ship.image.p, total, hipMemcpyDeviceToHost, ctx->stream));
        stamp(3);
        // the PN-Counter reads in front of the adds: the rows as they stood before the call, plus each read's prefix
        // (the read list holds at most n_reads entries: that sizes the grid; a batch without a read launches and copies nothing)
        const bool answer = ex && plan && n_reads != 0;
        std::vector<int64_t> hval(answer ? n : 0);
        std::vector<uint8_t> hovf(answer ? n : 0);
        const double t_tail = jg::now_us();
        if (answer) {
            jg::pnc_values_at_device(nd.pnc, col, rd.rrow, n_reads, sn.pdp, sn.pdn, rd.value, rd.ovf, rd.rat, rd.rcount, JG_Q_OVERFLOW);
            JG_HIP(hipMemcpyAsync(hval.data(), rd.value, n * 8, hipMemcpyDeviceToHost, ctx->stream));
            JG_HIP(hipMemcpyAsync(hovf.data(), rd.ovf, n, hipMemcpyDeviceToHost, ctx->stream));
        }
        if (nd.pnc) jg::pnc_add_list_device(nd.pnc, o.prow, o.pamt, o.pisn, o.count, n, col);
        if (guid) JG_HIP(hipMemcpyAsync(guid, o.guid, n * sizeof(jg_guid), hipMemcpyDeviceToHost, ctx->stream));
        JG_HIP(hipStreamSynchronize(ctx->stream));
        const double ms_tail = (jg::now_us() - t_tail) * 1e-3, t_out = jg::now_us();
        ship.bytes = total;
        ship.held = total != 0 && !fits;
        for (uint64_t i = 0; i < n; ++i)
            if (h_status[i] == JG_U_OK && h_kind[i] == 0 && !reads(i)) res[i] = 1;
        std::memcpy(status, h_status, n);
        if (ex) {
            for (uint64_t i = 0; i < n; ++i)
                if (answer && reads(i) && h_status[i] == JG_Q_OK && h_kind[i] == 0) {
                    val[i] = hval[i];
                    if (hovf[i]) status[i] = hovf[i];
                }
            std::memcpy(ex->value, val.data(), n * 8);
        }
        std::memcpy(result, res.data(), n);
        if (kind) std::memcpy(kind, h_kind, n);
        if (idx) std::memcpy(idx, h_idx, n * 4);
        if (elem) std::memcpy(elem, el.data(), n * 4);
        std::memcpy(snap_off, h_off, (n + 1) * 8);
        *n_bytes = total;
        if (sha && !total) std::memset(sha, 0, n * 32);
        if (n_rounds) *n_rounds = rounds;
        if (tr) {
            float mv = 0, hs = 0, cp = 0;
            JG_HIP(hipEventElapsedTime(&mv, ev[0], ev[1]));
            JG_HIP(hipEventElapsedTime(&hs, ev[1], ev[2]));
            JG_HIP(hipEventElapsedTime(&cp, ev[2], ev[3]));
            std::fprintf(stderr, "update_keys_ship(%llu commands, %llu OR-Set, %u rounds, %llu bytes): upload + resolve %.3f ms, OR-Set survivors %.3f ms, "
                         "PN-Counter plan %.3f ms, rounds on the host + dry size phase %.3f ms, applies %.3f ms, encodes %.3f ms, mover %.3f ms, "
                         "hashes %.3f ms, copy %.3f ms; behind them (by the host's clock) %llu reads' answers + adds + the wait for the stream %.3f ms, "
                         "outputs %.3f ms\n", (ull)n, (ull)n_o, rounds, (ull)total, ms_resolve, ms_surv, ms_pnc, ms_dry, ms_apply, ms_enc, mv, hs, cp,
                         (ull)n_reads, ms_tail, (jg::now_us() - t_out) * 1e-3);
            for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        }
    });
}

int node_shipped(jg_node* node, uint64_t* n_bytes, uint8_t* out, uint64_t cap) {
    return jg::guard([&] {
        JG_REQUIRE(node && n_bytes, JG_EINVAL, "jg_node_shipped: NULL argument");
        jg_ctx* ctx = jg::node_ctx(node);
        auto lk_ = jg::lock(ctx);
        jg::ShipState& ship = jg::node_ship(node);
        *n_bytes = ship.held ? ship.bytes : 0;
        if (!ship.held || !out) return;  // nothing held, or a size query
        JG_REQUIRE(ship.bytes <= cap, JG_ESTATE, "jg_node_shipped: %llu bytes exceed cap %llu (the image stays held)", (ull)ship.bytes, (ull)cap);
        jg::ensure_device(ctx);
        JG_HIP(hipMemcpyAsync(out, ship.image.p, ship.bytes, hipMemcpyDeviceToHost, ctx->stream));
        JG_HIP(hipStreamSynchronize(ctx->stream));
        ship.held = false;
    });
}

}  // namespace

extern "C" {

int jg_node_update_keys(jg_node* node, jg_keyspace* ks, uint64_t n, const uint64_t* key_off, const uint8_t* key_bytes, const uint8_t* op,
                        const uint8_t* arg_flag, const int64_t* amount, const uint64_t* elem_off, const uint8_t* elem_bytes, const uint64_t* tag_lo,
                        const uint64_t* tag_hi, uint32_t col, uint8_t* status, uint8_t* result, uint8_t* kind, uint32_t* idx, uint32_t* elem,
                        jg_guid* guid, uint64_t* add_lim, uint64_t* rem_lim) {
    return update_keys(node, ks, n, key_off, key_bytes, op, arg_flag, amount, elem_off, elem_bytes, tag_lo, tag_hi, col, status, result, kind, idx, elem,
                       guid, add_lim, rem_lim, nullptr);
}

int jg_node_update_keys_encode(jg_node* node, jg_keyspace* ks, uint64_t n, const uint64_t* key_off, const uint8_t* key_bytes, const uint8_t* op,
                               const uint8_t* arg_flag, const int64_t* amount, const uint64_t* elem_off, const uint8_t* elem_bytes,
                               const uint64_t* tag_lo, const uint64_t* tag_hi, uint32_t col, const uint8_t* snap, uint8_t* status, uint8_t* result,
                               uint8_t* kind, uint32_t* idx, uint32_t* elem, jg_guid* guid, uint64_t* add_lim, uint64_t* rem_lim, uint64_t* snap_off,
                               uint8_t* out, uint64_t cap, uint8_t* sha) {
    const Enc enc{snap, snap_off, out, cap, sha};
    return update_keys(node, ks, n, key_off, key_bytes, op, arg_flag, amount, elem_off, elem_bytes, tag_lo, tag_hi, col, status, result, kind, idx, elem,
                       guid, add_lim, rem_lim, &enc);
}

int jg_node_update_keys_ship(jg_node* node, jg_keyspace* ks, uint64_t n, const uint64_t* key_off, const uint8_t* key_bytes, const uint8_t* op,
                             const uint8_t* arg_flag, const int64_t* amount, const uint64_t* elem_off, const uint8_t* elem_bytes,
                             const uint64_t* tag_lo, const uint64_t* tag_hi, uint32_t col, const uint8_t* snap, uint8_t* status, uint8_t* result,
                             uint8_t* kind, uint32_t* idx, uint32_t* elem, jg_guid* guid, uint64_t* snap_off, uint64_t* n_bytes, uint8_t* out, uint64_t cap,
                             uint8_t* sha, uint32_t* n_rounds) {
    return update_keys_ship(node, ks, n, key_off, key_bytes, op, arg_flag, amount, elem_off, elem_bytes, tag_lo, tag_hi, col, snap, status, result, kind,
                            idx, elem, guid, snap_off, n_bytes, out, cap, sha, n_rounds);
}

int jg_node_exec_keys(jg_node* node, jg_keyspace* ks, uint64_t n, const uint64_t* key_off, const uint8_t* key_bytes, const uint8_t* cmd, const uint8_t* op,
                      const uint8_t* arg_flag, const int64_t* amount, const uint64_t* elem_off, const uint8_t* elem_bytes, const uint64_t* tag_lo,
                      const uint64_t* tag_hi, uint32_t col, const uint8_t* snap, uint8_t* status, uint8_t* result, int64_t* value, uint8_t* kind,
                      uint32_t* idx, uint32_t* elem, jg_guid* guid, uint64_t* snap_off, uint64_t* n_bytes, uint8_t* out, uint64_t cap, uint8_t* sha,
                      uint32_t* n_rounds) {
    const Exec ex{cmd, value};
    return update_keys_ship(node, ks, n, key_off, key_bytes, op, arg_flag, amount, elem_off, elem_bytes, tag_lo, tag_hi, col, snap, status, result, kind,
                            idx, elem, guid, snap_off, n_bytes, out, cap, sha, n_rounds, &ex);
}

int jg_node_shipped(jg_node* node, uint64_t* n_bytes, uint8_t* out, uint64_t cap) { return node_shipped(node, n_bytes, out, cap); }

}  // extern "C"
