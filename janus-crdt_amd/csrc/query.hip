// query.hip — client reads by key name, resolved on the device: jg_node_query_keys.
//
// The reference's "gp" / "gs" commands (CRDTCommands/PNCounterCommand.cs:27-41, ORSetCommand.cs:28-42) go
// KeySpaceManager.GetKVPair (KeySpaceManager.cs:138-142) -> SafeCRDT.QueryProspective / QueryStable (SafeCRDT.cs:64-78)
// -> PNCounter.Get (PNCounters.cs:87-90) or ORSet.Contains (ORSetWrapper.cs:24-28).  The three tables that chain is
// made of are resident already; this file only walks them in one call:
//
//   k_q_resolve  one lane per query: FNV-1a of the key -> dict_find in the key space's dictionary (tpset_dict.hpp)
//                -> uid_find in the node's uid table (uid_table.hpp, the probe k_classify runs) -> for an OR-Set read
//                with a string, name_key -> tab_find in the element table (orset_names.hpp).  Statuses NO_KEY,
//                NO_CRDT and NO_ARG are final here.  Each wave appends its resolved PN-Counter reads (row, query
//                index) to one list and its resolved OR-Set reads (set << 32 | id, query index) to another, with one
//                atomic per wave and list; the order inside a list is whatever the waves' atomics gave, the answers
//                are scattered back by query index, so the outputs do not depend on it.
//   answers      jg_pnc_values' kernel (one wave per key) over the first list, jg_orset_contains' kernel over the
//                second: both sized by the batch, both read their list's length from device memory, so no count
//                visits the host between resolve and answers and a batch of OR-Set reads launches no Get work.
//
// The three probes are a dependent chain of random lines: the kernel waits on memory, uses no LDS and few registers,
// so occupancy is what hides the latency.  Nothing is published inside a launch (no release / acquire between
// workgroups): the kernel boundaries publish the lists and their counts.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "launch.hpp"
#include "orset_names.hpp"
#include "tpset_dict.hpp"
#include "uid_table.hpp"
#include "wave_append.hpp"

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kNever = JG_NULL_ELEM - 1;  // "never allocated": the id no record carries (orset_names.hip)
using ull = unsigned long long;

struct QIn {  // the staged batch
    const ull *koff, *eoff;  // eoff / ebytes / flag NULL: no query carries an argument
    const uint8_t *kbytes, *ebytes, *flag;
};
struct QOut {
    long long* value;
    uint8_t *status, *kind;
    jg_guid* guid;
    uint32_t *prow, *pat;  // resolved PN-Counter reads: row, query index
    ull* oq;               // resolved OR-Set reads: set << 32 | element id
    uint32_t* oat;
    ull* count;  // [0] PN-Counter reads, [1] OR-Set reads (zeroed before the launch)
};

using jg::wave_append;

__global__ __launch_bounds__(kBlock) void k_q_resolve(jgt::Store S, jgt::Dict D, jg::DevUids U, uint64_t pnc_rows, jgn::Names N, uint64_t set_cap,
                                                      uint64_t kmask, uint64_t nsalt, QIn in, uint64_t n, QOut o) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    bool is_p = false, is_o = false;
    uint32_t row = 0;
    ull q = 0;
    if (i < n) {
        uint8_t st = JG_Q_NO_KEY, kd = 255;
        ull glo = 0, ghi = 0;
        const uint8_t* k = in.kbytes + in.koff[i];
        const uint32_t klen = (uint32_t)(in.koff[i + 1] - in.koff[i]);
        const uint32_t d = jgt::dict_find(S, D, jgt::key_hash(k, klen, S.salt), k, klen);
        if (d != jgt::kNone) {
            glo = D.glo[d], ghi = D.ghi[d];
            const uint32_t v = (glo | ghi) != 0 ? jg::uid_find(U, glo, ghi) : jg::kNoSlot;
            if (v == jg::kNoSlot) {
                st = JG_Q_NO_CRDT;
            } else if (!(v & jg::kOrSetBit)) {
                kd = 0;
                is_p = v < pnc_rows;  // jg_node_register checked the row and stores never shrink
                row = v;
                st = is_p ? JG_Q_OK : JG_Q_NO_CRDT;
            } else {
                kd = 1;
                const uint32_t set = v & ~jg::kOrSetBit;
                const uint32_t flag = in.flag ? in.flag[i] : 0;
                if (flag == 0) {
                    st = JG_Q_NO_ARG;
                } else {
                    uint32_t id = JG_NULL_ELEM;
                    if (flag == 1) {
                        id = jgn::kNoName;
                        if (set < set_cap) {  // a set the table never saw has no names
                            const uint8_t* b = in.ebytes + in.eoff[i];
                            const uint32_t len = (uint32_t)(in.eoff[i + 1] - in.eoff[i]);
                            uint64_t h = jgn::kFnvBasis;
                            for (uint32_t j = 0; j < len; ++j) h = (h ^ b[j]) * jgn::kFnvPrime;
                            id = jgn::tab_find(N, jgn::name_key(set, h, nsalt) & kmask, set, b, len);
                        }
                        if (id == jgn::kNoName) id = kNever;
                    }
                    q = (ull)set << 32 | id;
                    is_o = true;
                    st = JG_Q_OK;
                }
            }
        }
        o.value[i] = 0;
        o.status[i] = st;
        o.kind[i] = kd;
        if (o.guid) o.guid[i] = jg_guid{glo, ghi};
    }
    const ull sp = wave_append(is_p, o.count);
    if (is_p) o.prow[sp] = row, o.pat[sp] = (uint32_t)i;
    const ull so = wave_append(is_o, o.count + 1);
    if (is_o) o.oq[so] = q, o.oat[so] = (uint32_t)i;
}

void check_offsets(const char* what, uint64_t n, const uint64_t* off, const uint8_t* bytes) {
    JG_REQUIRE(off[0] == 0, JG_EINVAL, "jg_node_query_keys: %s_off[0] must be 0", what);
    for (uint64_t i = 0; i < n; ++i)
        JG_REQUIRE(off[i] <= off[i + 1] && off[i + 1] - off[i] < 0x7FFFFFFFull, JG_EINVAL, "jg_node_query_keys: %s offsets decrease at %llu", what,
                   (ull)i);
    JG_REQUIRE(off[n] == 0 || bytes, JG_EINVAL, "jg_node_query_keys: %s_bytes is NULL", what);
    JG_REQUIRE(off[n] < (1ull << 40), JG_EINVAL, "jg_node_query_keys: batch too large");
}

}  // namespace

extern "C" {

int jg_node_query_keys(jg_node* node, jg_keyspace* ks, uint64_t n, const uint64_t* key_off, const uint8_t* key_bytes, const uint64_t* elem_off,
                       const uint8_t* elem_bytes, const uint8_t* elem_flag, int64_t* value, uint8_t* status, uint8_t* kind, jg_guid* guid) {
    return jg::guard([&] {
        auto lk_ = jg::lock(ks);  // calls on one context are serialised (shared scratch, stream)
        if (n == 0) return;
        JG_REQUIRE(node && ks && value && status, JG_EINVAL, "jg_node_query_keys: NULL argument");
        JG_REQUIRE(jg::node_ctx(node) == ks->ctx, JG_EINVAL, "jg_node_query_keys: the key space and the node belong to different contexts");
        JG_REQUIRE(n < 0x7FFFFFF0ull, JG_EINVAL, "jg_node_query_keys: at most 2^31 queries per call");
        JG_REQUIRE(key_off, JG_EINVAL, "jg_node_query_keys: key_off is NULL");
        check_offsets("key", n, key_off, key_bytes);
        const int given = (elem_off != nullptr) + (elem_bytes != nullptr) + (elem_flag != nullptr);
        JG_REQUIRE(given == 0 || given == 3, JG_EINVAL, "jg_node_query_keys: elem_off, elem_bytes and elem_flag: all or none");
        const bool elems = given == 3;
        if (elems) {
            check_offsets("elem", n, elem_off, elem_bytes);
            for (uint64_t i = 0; i < n; ++i)
                JG_REQUIRE(elem_flag[i] <= 2, JG_EINVAL, "jg_node_query_keys: elem_flag[%llu] = %u (0 none, 1 string, 2 null)", (ull)i, elem_flag[i]);
        }
        jg_ctx* ctx = ks->ctx;
        jg::ensure_device(ctx);
        const jg::NodeRef nd = jg::node_query_ref(node, "jg_node_query_keys");  // pending registrations to the device
        jg::ElemTable none;  // a node without an OR-Set store: no name resolves
        jg::ElemTable* T = &none;
        if (nd.orset) {
            jg::sync_counts(nd.orset);
            T = jg::orset_elem_table(nd.orset, true);
            T->ensure_names(ctx, 0, 0);
        }

        // keys, elements, flags and offsets in one staging copy: koff | eoff | flag | key bytes | element bytes
        const uint64_t kb = key_off[n], eb = elems ? elem_off[n] : 0;
        QIn in{};
        QOut o{};
        jg::Layout L;
        L.add(in.koff, n + 1, 8), L.add(in.eoff, elems ? n + 1 : 0, 8), L.add(in.flag, elems ? n : 0, 1);
        L.add(in.kbytes, kb, 8), L.add(in.ebytes, eb, 1);
        const size_t stage = L.skip(0, 8);
        std::vector<uint8_t> h(stage);
        L.bind(h.data());  // the host image first: the same offsets as on the device
        std::memcpy(h.data(), key_off, (n + 1) * 8);
        if (kb) std::memcpy(const_cast<uint8_t*>(in.kbytes), key_bytes, kb);
        if (elems) {
            std::memcpy(const_cast<ull*>(in.eoff), elem_off, (n + 1) * 8);
            std::memcpy(const_cast<uint8_t*>(in.flag), elem_flag, n);
            if (eb) std::memcpy(const_cast<uint8_t*>(in.ebytes), elem_bytes, eb);
        }
        // behind it (16 bytes on): value | oq | count | guid | prow | pat | oat | status | kind
        L.skip(16);
        L.add(o.value, n), L.add(o.oq, n, 8), L.add(o.count, 2, 8), L.add(o.guid, guid ? n : 0, 8);
        L.add(o.prow, n, 4), L.add(o.pat, n, 4), L.add(o.oat, n, 4), L.add(o.status, n, 1), L.add(o.kind, n, 1);
        auto* d = static_cast<uint8_t*>(jg::scratch(ctx, ctx->scratch, L.bytes() + 64));
        L.bind(d);
        if (!elems) in.eoff = nullptr, in.ebytes = in.flag = nullptr;
        if (!guid) o.guid = nullptr;

        // JANUS_TRACE_QUERY (as JANUS_TRACE_APPLY): the upload, the launches and the copies out by hipEvents
        static const bool tr = std::getenv("JANUS_TRACE_QUERY") != nullptr;
        hipEvent_t ev[4] = {};
        auto stamp = [&](int k) {
            if (!tr) return;
            JG_HIP(hipEventCreate(&ev[k]));
            JG_HIP(hipEventRecord(ev[k], ctx->stream));
        };
        stamp(0);
        JG_HIP(hipMemcpyAsync(d, h.data(), stage, hipMemcpyHostToDevice, ctx->stream));
        stamp(1);
        JG_HIP(hipMemsetAsync(o.count, 0, 16, ctx->stream));
        hipLaunchKernelGGL(k_q_resolve, dim3(jg::blocks_for(n)), dim3(kBlock), 0, ctx->stream, ks->set->view(), ks->dict(), nd.uids,
                           nd.pnc ? nd.pnc->n_keys : 0, T->view(), T->set_cap, T->kmask, T->salt, in, n, o);
        JG_HIP(hipGetLastError());
        if (nd.pnc) jg::pnc_values_device(nd.pnc, o.prow, n, o.value, o.status, o.pat, o.count, JG_Q_OVERFLOW);
        if (nd.orset) jg::orset_contains_device(nd.orset, o.oq, n, nullptr, o.oat, o.count + 1, o.value);
        stamp(2);
        JG_HIP(hipMemcpyAsync(value, o.value, n * 8, hipMemcpyDeviceToHost, ctx->stream));
        JG_HIP(hipMemcpyAsync(status, o.status, n, hipMemcpyDeviceToHost, ctx->stream));
        if (kind) JG_HIP(hipMemcpyAsync(kind, o.kind, n, hipMemcpyDeviceToHost, ctx->stream));
        if (guid) JG_HIP(hipMemcpyAsync(guid, o.guid, n * sizeof(jg_guid), hipMemcpyDeviceToHost, ctx->stream));
        stamp(3);
        JG_HIP(hipStreamSynchronize(ctx->stream));
        if (tr) {
            float up = 0, run = 0, down = 0;
            JG_HIP(hipEventElapsedTime(&up, ev[0], ev[1]));
            JG_HIP(hipEventElapsedTime(&run, ev[1], ev[2]));
            JG_HIP(hipEventElapsedTime(&down, ev[2], ev[3]));
            std::fprintf(stderr, "query_keys(%llu queries, %llu bytes up, %llu bytes down): upload %.3f ms, resolve + answer launches %.3f ms, "
                         "copies out %.3f ms\n", (ull)n, (ull)stage, (ull)(n * (10 + (guid ? 16 : 0))), up, run, down);
            for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        }
    });
}

}  // extern "C"
