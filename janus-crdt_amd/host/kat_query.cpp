// host/kat_query.cpp — client reads by key name on the device against the oracle's SafeCRDT.QueryProspective /
// QueryStable (BFT-CRDT/SafeCRDTs/SafeCRDT.cs:64-78), in kat_keyspace's scenario: four nodes, each a key space, a
// prospective and a stable copy on one context.  Node 0 creates the keys; the others learn them through Receive and
// create the CRDTs from the callback.  Every node then takes client ops on its prospective copies (SafeCRDT.Update)
// and merges the other nodes' blocks into them (ReceivedBlock); one committed wave carries every submitted state to
// the stable copies.  Every node answers "gp" and "gs" for every key BY NAME (janus::QueryKeys, one
// jg_node_query_keys per copy), every OR-Set key with a member, a non-member and null: before the wave "gs" lags "gp",
// after it they agree on every node (KVStoreTests.cs:225-286).  Prints "PASS name" / "FAIL name: why" like kat_device.
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
void expect(bool ok, const std::string& what) {
    if (!ok) throw std::runtime_error(what);
}

jg_ctx* g_ctx;

janus::CrdtType type_of(const std::string& key) { return key.compare(0, 3, "pnc") == 0 ? janus::CrdtType::PNCounter : janus::CrdtType::ORSet; }

struct Node {
    int id;
    janus::GpuKeySpace ks;
    janus::GpuStableStore stable, prospective;
    oracle::SafeCRDTManager sm;  // the reference's node: both copies of every key
    uint64_t tags = 0;
    explicit Node(int i) : id(i), ks(g_ctx, 256, 1 << 16), stable(g_ctx, 256, 8, 4), prospective(g_ctx, 256, 8, 4), sm(1, 0x9000 + (uint64_t)i) {}

    void create_crdt(const std::string& key, const jg_guid& g) {
        const janus::Guid uid{g.lo, g.hi};
        stable.CreateSafeCRDT(uid, type_of(key), janus::Guid{0x57AB1E00ull + (uint64_t)id, 1});
        prospective.CreateSafeCRDT(uid, type_of(key), janus::Guid{0x9405900ull + (uint64_t)id, 2});
        sm.CreateSafeCRDT(key, type_of(key) == janus::CrdtType::PNCounter ? oracle::CrdtType::PNCounter : oracle::CrdtType::ORSet, oracle::Guid{g.lo, g.hi});
    }
    // SafeCRDT.Update on the oracle (its snapshot goes to sm.submitted) and the same op on the device's prospective copy
    void update(const std::string& key, int op, const oracle::Arg& arg) {
        oracle::SafeCRDT& c = *sm.safeCRDTs.at(key);
        c.Update(op, {arg}, false);
        janus::ClientOp o;
        o.uid = janus::Guid{c.guid.lo, c.guid.hi};
        o.opId = op;
        o.amount = arg.i;
        if (arg.kind == oracle::Arg::Str) o.elem = arg.s;
        o.tag = janus::Guid{0x7A600000ull + (uint64_t)id, ++tags};
        (void)prospective.ApplyOps(std::vector<janus::ClientOp>{o});
    }
};

std::string member_of(const std::string& key) { return "m-" + key; }

// "gp" and "gs" of every key by name on one node, against the oracle; returns how many answers of the two copies differ
size_t read_all(Node& n, const std::vector<std::string>& keys) {
    std::vector<janus::KeyQuery> q;
    std::vector<std::vector<oracle::Arg>> args;
    for (const std::string& k : keys) {
        if (type_of(k) == janus::CrdtType::PNCounter) {
            q.push_back(janus::KeyQuery{k, false, std::nullopt});
            args.push_back({});
        } else {
            for (const auto& e : {std::optional<std::string>(member_of(k)), std::optional<std::string>("never"), std::optional<std::string>()}) {
                q.push_back(janus::KeyQuery{k, true, e});
                args.push_back({e ? oracle::Arg::S(*e) : oracle::Arg::N()});
            }
        }
    }
    q.push_back(janus::KeyQuery{"absent", false, std::nullopt});
    const std::vector<janus::KeyAnswer> gp = janus::QueryKeys(n.ks, n.prospective, q), gs = janus::QueryKeys(n.ks, n.stable, q);
    size_t differ = 0;
    for (size_t i = 0; i + 1 < q.size(); ++i) {
        const oracle::SafeCRDT& c = *n.sm.safeCRDTs.at(q[i].key);
        const oracle::Result wp = c.QueryProspective(args[i]), ws = c.QueryStable(args[i]);
        const bool pnc = c.type == oracle::CrdtType::PNCounter;
        const std::string at = "node " + std::to_string(n.id) + " key " + q[i].key;
        expect(gp[i].status == JG_Q_OK && gs[i].status == JG_Q_OK, at + ": status");
        expect(gp[i].kind == (pnc ? 0 : 1) && gs[i].kind == gp[i].kind, at + ": kind");
        expect(gp[i].guid == janus::Guid{c.guid.lo, c.guid.hi} && gs[i].guid == gp[i].guid, at + ": guid");
        expect(gp[i].value == (pnc ? wp.i : (int64_t)wp.b), at + ": \"gp\" equals QueryProspective");
        expect(gs[i].value == (pnc ? ws.i : (int64_t)ws.b), at + ": \"gs\" equals QueryStable");
        differ += gp[i].value != gs[i].value;
    }
    expect(gp.back().status == JG_Q_NO_KEY && gs.back().status == JG_Q_NO_KEY && gp.back().kind == 255, "an unknown key is JG_Q_NO_KEY");
    return differ;
}

void FourNodeReadsByName() {
    std::vector<std::unique_ptr<Node>> node;
    for (int i = 0; i < 4; ++i) node.emplace_back(new Node(i));
    std::vector<std::string> keys;
    std::vector<std::string> states;
    for (uint64_t k = 0; k < 12; ++k) {
        keys.push_back((k % 2 ? "orset" : "pnc") + std::to_string(k));
        const jg_guid g{0x2000 + k, 0xFEDCBA0000000000ull + k * 31};
        expect(node[0]->ks.CreateNewKVPair(keys.back(), g), "CreateNewKVPair");
        node[0]->create_crdt(keys.back(), g);
    }
    states.push_back(node[0]->ks.Encode());
    for (int i = 1; i < 4; ++i)
        expect(node[i]->ks.Receive(states, [&](const std::string& k, const jg_guid& g) { node[i]->create_crdt(k, g); }) == -1, "Receive");

    // client ops on every node's prospective copies
    for (int i = 0; i < 4; ++i) {
        Node& n = *node[i];
        for (size_t k = 0; k < keys.size(); ++k) {
            const std::string& key = keys[k];
            if (type_of(key) == janus::CrdtType::PNCounter) {
                n.update(key, 1, oracle::Arg::I(10 + 3 * (int)k + i));
                if ((k + i) % 3 == 0) n.update(key, 2, oracle::Arg::I(1 + i));
            } else {
                if ((k + i) % 2 == 0) n.update(key, 1, oracle::Arg::S(member_of(key)));
                n.update(key, 1, oracle::Arg::S("gone"));
                if (i == 1) n.update(key, 2, oracle::Arg::S("gone"));
                if (k % 3 == 0 && i == 2) n.update(key, 1, oracle::Arg::N());
            }
        }
    }
    // every node's blocks reach the other nodes' prospective copies (ReceivedBlock; RM:290-344)
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            if (i == j) continue;
            std::vector<janus::UpdateMessage> block;
            for (const oracle::UpdateMessage& um : node[j]->sm.submitted) {
                janus::UpdateMessage b;
                for (const oracle::NetworkProtocol& np : um.update) {
                    janus::NetworkProtocol m;
                    m.uid = janus::Guid{np.uid.lo, np.uid.hi};
                    m.message = np.bytes;
                    b.update.push_back(m);
                    oracle::SafeCRDT& c = *node[i]->sm.safeCRDTsIndexedByuid.at(np.uid);
                    if (c.type == oracle::CrdtType::PNCounter) c.pncProspective->pnc.Merge(oracle::json::DecodePNC<int32_t>(np.bytes));
                    else c.orProspective->orset.Merge(oracle::json::DecodeORSet(np.bytes));
                }
                block.push_back(b);
            }
            node[i]->prospective.ReceivedBlock(block);
        }
    for (int i = 0; i < 4; ++i) expect(read_all(*node[i], keys) > 0, "before the wave \"gs\" lags \"gp\"");

    // one committed wave: every node's submitted messages, in node order, to every stable copy
    std::vector<std::vector<janus::UpdateMessage>> wave(1);
    std::vector<std::vector<oracle::UpdateMessage>> owave(1);
    for (int j = 0; j < 4; ++j)
        for (const oracle::UpdateMessage& um : node[j]->sm.submitted) {
            owave[0].push_back(um);
            janus::UpdateMessage b;
            for (const oracle::NetworkProtocol& np : um.update) {
                janus::NetworkProtocol m;
                m.uid = janus::Guid{np.uid.lo, np.uid.hi};
                m.message = np.bytes;
                b.update.push_back(m);
            }
            wave[0].push_back(b);
        }
    for (int i = 0; i < 4; ++i) {
        node[i]->stable.ApplyCommitted(wave);
        node[i]->sm.HandleAfterConsensusUpdates(owave);
        expect(read_all(*node[i], keys) == 0, "after the wave \"gs\" and \"gp\" agree");
    }
}

}  // namespace

int main() {
    check(jg_open(0, &g_ctx), "jg_open");
    const std::vector<std::pair<std::string, std::function<void()>>> tests = {{"Query.FourNodeReadsByName", FourNodeReadsByName}};
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
