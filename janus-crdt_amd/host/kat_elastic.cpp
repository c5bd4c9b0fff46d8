// host/kat_elastic.cpp — four nodes whose PN-Counter stores start at 2 keys x 2 replica columns and grow on the
// device (GpuStableStore::SetElastic over jg_pnc_reserve / jg_pnc_set_max_replicas): they learn 8 keys through
// janus::GpuKeySpace::Receive, create the counters from the callback (the key capacity doubles 2 -> 4 -> 8) and apply
// one committed wave in which every key carries the four nodes' replicas and one more (5 columns: 2 -> 4 -> 8),
// checked against the oracle's PNCounter — whose Dictionaries take any number of keys and replicas
// (KeySpaceManager.cs:121-136, PNCounters.cs:131-144).  Prints "PASS name" / "FAIL name: why" like kat_keyspace;
// exit 0 = every scenario passes.
#include <cstdio>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "janus_host.hpp"
#include "json.hpp"
#include "keyspace.hpp"
#include "oracle.hpp"

namespace {

void check(int rc, const char* what) {
    if (rc == JG_OK) return;
    char buf[512];
    jg_last_error(buf, sizeof buf);
    throw std::runtime_error(std::string(what) + ": " + buf);
}
void expect(bool ok, const char* what) {
    if (!ok) throw std::runtime_error(what);
}

jg_ctx* g_ctx;

janus::Guid replica_of(int i) { return janus::Guid{0x5E1F0000ull + (uint64_t)i, 0x0DE0 + (uint64_t)i}; }

struct Node {
    janus::GpuKeySpace ks;
    janus::GpuStableStore store;
    janus::Guid replica;
    explicit Node(int i, bool elastic = true) : ks(g_ctx, 256, 1 << 16), store(0, 2, 2, 4), replica(replica_of(i)) {
        if (elastic) store.SetElastic(64, 16);
    }
    void create_crdt(const jg_guid& g) { store.CreateSafeCRDT(janus::Guid{g.lo, g.hi}, janus::CrdtType::PNCounter, replica); }
    void shape(uint64_t* nk, uint32_t* r) {
        uint32_t eb = 0;
        check(jg_pnc_shape(store.pnc(), nk, r, &eb), "jg_pnc_shape");
        expect(eb == 4, "the width stays");
    }
};

void FixedStoreStaysFull() {  // never asked: today's errors
    Node n(0, false);
    n.create_crdt(jg_guid{1, 1});
    n.create_crdt(jg_guid{2, 2});
    try {
        n.create_crdt(jg_guid{3, 3});
    } catch (const janus::EngineError& e) {
        expect(e.code == JG_ESTATE && std::string(e.what()) == "PNCounter store full", "the fixed store's error");
        uint64_t nk;
        uint32_t r;
        n.shape(&nk, &r);
        expect(nk == 2 && r == 2, "the fixed store's shape");
        return;
    }
    expect(false, "a fixed store took a third key");
}

void FourNodesGrowKeysAndColumns() {
    std::vector<std::unique_ptr<Node>> node;
    for (int i = 0; i < 4; ++i) node.emplace_back(new Node(i));
    std::vector<std::pair<std::string, jg_guid>> made;
    for (uint64_t k = 0; k < 8; ++k) made.push_back({"pnc" + std::to_string(k), jg_guid{0x2000 + k, 0xABCDEF0000000000ull + k * 91}});
    for (const auto& m : made) {
        expect(node[0]->ks.CreateNewKVPair(m.first, m.second), "CreateNewKVPair's TryAdd");
        node[0]->create_crdt(m.second);
    }
    const std::vector<std::string> states{node[0]->ks.Encode()};
    for (int i = 1; i < 4; ++i) {
        size_t learnt = 0;
        expect(node[i]->ks.Receive(states, [&](const std::string&, const jg_guid& g) {
            node[i]->create_crdt(g);  // past the second key this grows the store: 2 -> 4 -> 8
            ++learnt;
        }) == -1, "Receive's verdict");
        expect(learnt == made.size(), "every key of node 0 is learnt once");
    }
    for (int i = 0; i < 4; ++i) {
        uint64_t nk;
        uint32_t r;
        node[i]->shape(&nk, &r);
        expect(nk == 8 && r == 2, "8 keys x 2 columns after the keys were created");
        expect(node[i]->store.MaxKeys() == 8 && node[i]->store.Replicas() == 2, "the mirror follows jg_pnc_shape");
    }

    // one committed wave: every key's state names one replica of its own and the four nodes' (5 columns a key)
    std::vector<std::vector<janus::UpdateMessage>> wave(1);
    std::vector<std::string> state_of;
    janus::UpdateMessage um;
    for (uint64_t k = 0; k < made.size(); ++k) {
        oracle::PNCounter<int32_t> src(oracle::Guid{0xABC000 + k, 0x51C});
        src.Increment((int32_t)(10 + 3 * k));
        src.Decrement((int32_t)(k % 4));
        for (int i = 0; i < 4; ++i) {
            const janus::Guid r = replica_of((int)((i + k) % 4));  // the nodes' replicas in an order of the key's own
            oracle::PNCounter<int32_t> peer(oracle::Guid{r.lo, r.hi});
            peer.Increment((int32_t)(100 * (i + 1) + k));
            peer.Decrement((int32_t)(7 * i + 1));
            src.Merge(peer.GetLastSynchronizedUpdate());
        }
        state_of.push_back(oracle::json::EncodePNC(src.GetLastSynchronizedUpdate()));
        janus::NetworkProtocol np;
        np.uid = janus::Guid{made[k].second.lo, made[k].second.hi};
        np.message = state_of.back();
        um.update.push_back(np);
        if (um.update.size() == 3 || k + 1 == made.size()) {
            wave[0].push_back(um);
            um = janus::UpdateMessage();
        }
    }
    for (int i = 0; i < 4; ++i) {
        Node& n = *node[i];
        n.store.ApplyCommitted(wave);  // a key out of columns widens the store instead of cutting the wave
        uint64_t nk;
        uint32_t r;
        n.shape(&nk, &r);
        expect(nk == 8 && r == 8, "jg_pnc_shape reports 8 x 8");
        expect(n.store.Replicas() == 8, "the mirror follows the widening");
        std::vector<janus::Guid> uids;
        std::vector<std::string> want_state;
        for (uint64_t k = 0; k < made.size(); ++k) {
            const janus::Guid uid{made[k].second.lo, made[k].second.hi};
            oracle::PNCounter<int32_t> want(oracle::Guid{n.replica.lo, n.replica.hi});
            want.Merge(oracle::json::DecodePNC<int32_t>(state_of[k]));
            expect(n.store.QueryStablePNC(uid) == (int64_t)want.Get(), "QueryStablePNC equals the oracle's Get");
            uids.push_back(uid);
            want_state.push_back(oracle::json::EncodePNC(want.GetLastSynchronizedUpdate()));
        }
        // the encoded states carry the replicas in column order: byte-equal = the Dictionary's enumeration order
        expect(n.store.EncodePNCStates(uids) == want_state, "the encoded states (values, column order) equal the oracle's");
    }
}

}  // namespace

int main() {
    check(jg_open(0, &g_ctx), "jg_open");
    const std::vector<std::pair<std::string, std::function<void()>>> tests = {
        {"Elastic.FixedStoreStaysFull", FixedStoreStaysFull}, {"Elastic.FourNodesGrowKeysAndColumns", FourNodesGrowKeysAndColumns}};
    int failed = 0;
    for (const auto& t : tests) {
        try {
            t.second();
            std::printf("PASS %s\n", t.first.c_str());
        } catch (const std::exception& e) {
            std::printf("FAIL %s: %s\n", t.first.c_str(), e.what());
            ++failed;
        }
    }
    (void)jg_close(g_ctx);
    return failed ? 1 : 0;
}
