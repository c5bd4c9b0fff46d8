// host/kat_keyspace.cpp — the reference's TPSet scenarios (MergeSharp.Tests/2PSetTests.cs) replayed on the device
// with their literal asserts, and four nodes that learn each other's keys through janus::GpuKeySpace (checked against
// host/tpset_ref.hpp's OnNext), create the CRDTs from the callback and apply one committed wave (checked against the oracle).  Prints "PASS name" /
// "FAIL name: why" like kat_device; exit 0 = every scenario passes.
#include <cstdio>
#include <functional>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "janus_host.hpp"
#include "json.hpp"
#include "keyspace.hpp"
#include "oracle.hpp"
#include "tpset_ref.hpp"

namespace {

using Strs = std::vector<std::string>;

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

struct DevTPSet {  // TPSet<string> on the device
    jg_tpset* s = nullptr;
    DevTPSet() { check(jg_tpset_create(g_ctx, 64, 4096, &s), "jg_tpset_create"); }
    ~DevTPSet() { (void)jg_tpset_destroy(s); }
    bool op(uint8_t id, const std::string& x) {
        const uint64_t off[2] = {0, x.size()};
        uint8_t r = 0;
        check(jg_tpset_apply_ops(s, 1, &id, off, reinterpret_cast<const uint8_t*>(x.data()), nullptr, &r), "jg_tpset_apply_ops");
        return r != 0;
    }
    void Add(const std::string& x) { op(1, x); }
    bool Remove(const std::string& x) { return op(2, x); }
    long Count() {
        uint64_t a, r, b;
        check(jg_tpset_size(s, &a, &r, &b), "jg_tpset_size");
        return (long)a - (long)r;
    }
    Strs LookupAll() {
        uint64_t n = 0, nb = 0;
        check(jg_tpset_lookup_all(s, 0, &n, &nb, nullptr, nullptr, nullptr, nullptr), "jg_tpset_lookup_all");
        std::vector<uint64_t> ord(n + 1), off(n + 1);
        std::string bytes(nb + 1, '\0');
        std::vector<uint8_t> nul(n + 1);
        check(jg_tpset_lookup_all(s, 0, &n, &nb, ord.data(), off.data(), reinterpret_cast<uint8_t*>(bytes.data()), nul.data()), "jg_tpset_lookup_all");
        Strs out;
        for (uint64_t i = 0; i < n; ++i) out.push_back(bytes.substr(off[i], off[i + 1] - off[i]));
        return out;
    }
    std::string Encode() {
        uint64_t n = 0;
        check(jg_tpset_encode_json(s, &n, nullptr, 0), "jg_tpset_encode_json");
        std::string out(n, '\0');
        check(jg_tpset_encode_json(s, &n, reinterpret_cast<uint8_t*>(out.data()), n), "jg_tpset_encode_json");
        return out;
    }
    void Merge(const std::string& wire) {  // Decode + Merge of an encoded TPSetMsg
        const uint64_t off[2] = {0, wire.size()};
        uint64_t bad;
        uint8_t partial;
        check(jg_tpset_merge_json(s, 1, off, reinterpret_cast<const uint8_t*>(wire.data()), 0, &bad, &partial), "jg_tpset_merge_json");
    }
};

void TestTPsetSingle() {
    DevTPSet set;
    set.Add("a");
    set.Add("b");
    set.Remove("a");
    expect(!set.Remove("c"), "Assert.False(set.Remove(\"c\"))");
    set.Add("c");
    expect(set.Count() == 2, "Assert.Equal(2, set.Count)");
    expect(set.LookupAll() == Strs{"b", "c"}, "LookupAll == {b, c}");
}
void TestTPsetMerge() {  // also TPSetMsgTests.EncodeDecode: the state crosses the wire
    DevTPSet set, set2;
    set.Add("a");
    set.Add("b");
    set2.Add("c");
    set2.Add("d");
    set2.Remove("c");
    const std::string wire = set2.Encode();
    expect(wire == "{\"addSet\":[\"c\",\"d\"],\"removeSet\":[\"c\"]}", "Encode of set2");
    set.Merge(wire);
    expect(set.LookupAll() == Strs{"a", "b", "d"}, "LookupAll == {a, b, d}");
}
void TrueEquals() {
    DevTPSet set, set2;
    set.Add("a"), set.Add("b"), set2.Add("a"), set2.Add("b");
    expect(set.LookupAll() == set2.LookupAll(), "Assert.True(set.Equals(set2))");
}
void FalseEquals() {
    DevTPSet set, set2;
    set.Add("a"), set.Add("b"), set2.Add("c");
    expect(set.LookupAll() != set2.LookupAll(), "Assert.False(set.Equals(set2))");
}

// Four nodes, each a key space (with its C++ restatement beside it) and a stable store.  Node 0 creates PN-Counter
// and OR-Set keys; nodes 1-3 learn them only through Receive on node 0's encoded states and create the CRDTs from the
// callback (the caller supplies the type: here the key's prefix stands for what the replication manager tells the
// reference, SafeCRDTManager.cs:88).  Node 2 created "pnc4" itself first and keeps its own guid for it.  One committed
// wave with a state for every uid node 0 made is then applied on all four through ApplyCommitted, and every node's
// QueryStable* must equal the oracle's CRDT of that node merged with the same state.
struct Node {
    janus::GpuKeySpace ks;
    janus::ref::KeySpace ref;
    janus::GpuStableStore store;
    janus::Guid replica;
    size_t journal_at = 0;
    explicit Node(int i) : ks(g_ctx, 256, 1 << 16), store(0, 256, 8, 4), replica{0x5E1F0000ull + (uint64_t)i, 0x0DE0 + (uint64_t)i} {}
    static janus::CrdtType type_of(const std::string& key) { return key.compare(0, 3, "pnc") == 0 ? janus::CrdtType::PNCounter : janus::CrdtType::ORSet; }
    void create_crdt(const std::string& key, const jg_guid& g) { store.CreateSafeCRDT(janus::Guid{g.lo, g.hi}, type_of(key), replica); }
    void create(const std::string& key, const jg_guid& g, bool want) {
        expect(ks.CreateNewKVPair(key, g) == want, "CreateNewKVPair's TryAdd");
        expect(ref.CreateNewKVPair(key, oracle::Guid{g.lo, g.hi}) == want, "the restatement's TryAdd");
        if (want) create_crdt(key, g);
    }
    // Receive on the device and on the restatement: the same verdict, the same new keys in the same order
    void receive(const std::vector<std::string>& states, long want_bad) {
        std::vector<std::pair<std::string, jg_guid>> got;
        const long bad = ks.Receive(states, [&](const std::string& k, const jg_guid& g) {
            got.push_back({k, g});
            create_crdt(k, g);
        });
        expect(bad == want_bad, "Receive's verdict");
        for (size_t m = 0; m < states.size(); ++m) {
            const int st = ref.Receive(states[m]);
            expect((st != 0) == ((long)m == want_bad), "the restatement's verdict");
            if (st) break;
        }
        size_t at = 0;
        for (; journal_at < ref.journal().size(); ++journal_at) {
            const auto& r = ref.journal()[journal_at];
            if (r.status != 0) continue;
            expect(at < got.size() && got[at].first == r.bytes && got[at].second.lo == r.guid.lo && got[at].second.hi == r.guid.hi,
                   "new keys equal OnNext's, in order");
            ++at;
        }
        expect(at == got.size(), "no other key is journalled");
        expect(ks.Encode() == ref.set().Encode(), "the set's encoded state equals the restatement's");
        for (const auto& kv : ref.keys()) {
            const auto g = ks.Lookup(kv.first);
            expect(g && g->lo == kv.second.lo && g->hi == kv.second.hi, "Lookup equals keySpaces[key]");
        }
        expect(!ks.Lookup("absent"), "Lookup of an unknown key");
    }
};

void FourNodeKeyDiscoveryAndApply() {
    std::vector<std::unique_ptr<Node>> node;
    for (int i = 0; i < 4; ++i) node.emplace_back(new Node(i));
    std::vector<std::pair<std::string, jg_guid>> made;
    for (uint64_t k = 0; k < 20; ++k) made.push_back({(k % 2 ? "orset" : "pnc") + std::to_string(k), jg_guid{0x1000 + k, 0xABCDEF0000000000ull + k * 77}});
    node[2]->create("pnc4", jg_guid{7, 7}, true);
    std::vector<std::string> states;
    for (const auto& m : made) {
        node[0]->create(m.first, m.second, true);
        if (states.size() < 3 || &m == &made.back()) states.push_back(node[0]->ks.Encode());  // full states, as the reference ships them
    }
    node[0]->create("pnc0", jg_guid{9, 9}, false);
    for (int i = 1; i < 4; ++i) {
        node[i]->receive(states, -1);
        expect(node[i]->ref.journal().size() == (i == 2 ? made.size() - 1 : made.size()), "every key of node 0 is learnt once");
        node[i]->receive(states, -1);  // a state received again adds nothing
    }
    node[1]->receive({"{\"addSet\":[\"orsetlate\\u0000" "00000000-0000-0000-0000-0000000000aa\"],\"removeSet\":[]}", "{\"addSet\":[1]}"}, 1);
    expect(node[1]->ks.Lookup("orsetlate")->hi == 0xAA00000000000000ull, "the key before the rejected message is learnt");

    // one committed wave: a state for every uid node 0 made, from a replica none of the four is
    std::vector<std::vector<janus::UpdateMessage>> wave(1);
    std::map<std::string, std::string> state_of;
    janus::UpdateMessage um;
    for (uint64_t k = 0; k < made.size(); ++k) {
        std::string bytes;
        if (Node::type_of(made[k].first) == janus::CrdtType::PNCounter) {
            oracle::PNCounter<int32_t> src(oracle::Guid{0xABC000 + k, 0x51C});
            src.Increment((int32_t)(10 + 3 * k));
            src.Decrement((int32_t)(k % 4));
            bytes = oracle::json::EncodePNC(src.GetLastSynchronizedUpdate());
        } else {
            oracle::ORSet src;
            src.AddTag(std::string("e") + std::to_string(k), oracle::Guid{0x7A6000 + k, 1});
            src.AddTag(std::string("gone\"\\"), oracle::Guid{0x7A6000 + k, 2});
            src.Remove(std::string("gone\"\\"));
            if (k % 3 == 0) src.AddTag(std::nullopt, oracle::Guid{0x7A6000 + k, 3});
            bytes = oracle::json::EncodeORSet(src.GetLastSynchronizedUpdate());
        }
        state_of[made[k].first] = bytes;
        janus::NetworkProtocol np;
        np.uid = janus::Guid{made[k].second.lo, made[k].second.hi};
        np.message = bytes;
        um.update.push_back(np);
        if (um.update.size() == 7 || k + 1 == made.size()) {
            wave[0].push_back(um);
            um = janus::UpdateMessage();
        }
    }
    for (int i = 0; i < 4; ++i) {
        Node& n = *node[i];
        n.store.ApplyCommitted(wave);
        for (const auto& m : made) {
            const bool own = i == 2 && m.first == "pnc4";  // node 2 holds pnc4 under its own guid: the wave's state is not its
            const jg_guid g = *n.ks.Lookup(m.first);
            expect(own ? (g.lo == 7 && g.hi == 7) : (g.lo == m.second.lo && g.hi == m.second.hi), "the uid the key resolves to");
            const janus::Guid uid{g.lo, g.hi};
            if (Node::type_of(m.first) == janus::CrdtType::PNCounter) {
                oracle::PNCounter<int32_t> want(oracle::Guid{n.replica.lo, n.replica.hi});
                if (!own) want.Merge(oracle::json::DecodePNC<int32_t>(state_of[m.first]));
                expect(n.store.QueryStablePNC(uid) == (int64_t)want.Get(), "QueryStablePNC equals the oracle's Get");
            } else {
                oracle::ORSet want;
                want.Merge(oracle::json::DecodeORSet(state_of[m.first]));
                expect(n.store.QueryStableLookupAll(uid) == want.LookupAll(), "QueryStableLookupAll equals the oracle's");
                for (const oracle::Elem& e : {oracle::Elem("e" + m.first.substr(5)), oracle::Elem("gone\"\\"), oracle::Elem(std::nullopt), oracle::Elem("never")})
                    expect(n.store.QueryStableORSet(uid, e) == want.Contains(e), "QueryStableORSet equals the oracle's Contains");
            }
        }
    }
}

}  // namespace

int main() {
    check(jg_open(0, &g_ctx), "jg_open");
    const std::vector<std::pair<std::string, std::function<void()>>> tests = {
        {"TPSetTests.TestTPsetSingle", TestTPsetSingle}, {"TPSetTests.TestTPsetMerge+TPSetMsgTests.EncodeDecode", TestTPsetMerge},
        {"TPSetTests.TrueEquals", TrueEquals},           {"TPSetTests.FalseEquals", FalseEquals},
        {"KeySpace.FourNodeKeyDiscoveryAndApply", FourNodeKeyDiscoveryAndApply}};
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
