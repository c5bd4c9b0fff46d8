// host/kat_update.cpp — client writes by key name on the device against the oracle's SafeCRDT.Update
// (BFT-CRDT/SafeCRDTs/SafeCRDT.cs:39-47), in kat_query's scenario: four nodes, each a key space, a prospective and a
// stable copy on one context.  Node 0 creates the keys; the others learn them through Receive and create the CRDTs from
// the callback.  Every node then takes one scripted batch of commands BY KEY NAME on its prospective copy
// (janus::UpdateKeys, one jg_node_update_keys): PN-Counter increments and decrements, OR-Set Add / Remove / Clear, the
// null element, an unknown key, arguments of the wrong type, no argument and operation ids no wrapper knows.  Per
// command its status and result are the oracle's (the exception it throws, or Update's bool); afterwards every key's
// "gp" equals QueryProspective and every key's encoded state equals GetLastSynchronizedUpdate().Encode() byte for byte,
// while "gs" stays as it was until a committed wave carries the submitted states to the stable copies.  A round of ops
// through the mirror's own path (ApplyOps) on the sets the batch Cleared checks that the mirror recorded the Clears.
// Prints "PASS name" / "FAIL name: why" like kat_device.
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
std::string g_differing;  // read_all: the answers on which the two copies differed (for the failure message)

janus::Guid G(const oracle::Guid& g) { return janus::Guid{g.lo, g.hi}; }
janus::CrdtType type_of(const std::string& key) { return key.compare(0, 3, "pnc") == 0 ? janus::CrdtType::PNCounter : janus::CrdtType::ORSet; }

struct Command {
    std::string key;
    int op;
    bool has_arg;
    oracle::Arg arg;
};

struct Node {
    int id;
    janus::GpuKeySpace ks;
    janus::GpuStableStore stable, prospective;
    oracle::SafeCRDTManager sm;  // the reference's node: both copies of every key
    explicit Node(int i) : id(i), ks(g_ctx, 256, 1 << 16), stable(g_ctx, 256, 8, 4), prospective(g_ctx, 256, 8, 4), sm(1, 0x9000 + (uint64_t)i) {}

    // the oracle's CRDT first: the device copies take its replica Guids, so the encoded states can be compared
    void create_crdt(const std::string& key, const jg_guid& g) {
        const bool pnc = type_of(key) == janus::CrdtType::PNCounter;
        oracle::SafeCRDT& c = sm.CreateSafeCRDT(key, pnc ? oracle::CrdtType::PNCounter : oracle::CrdtType::ORSet, oracle::Guid{g.lo, g.hi});
        const janus::Guid uid{g.lo, g.hi};
        stable.CreateSafeCRDT(uid, type_of(key), pnc ? G(c.pncStable->pnc.replicaIdx()) : janus::Guid{});
        prospective.CreateSafeCRDT(uid, type_of(key), pnc ? G(c.pncProspective->pnc.replicaIdx()) : janus::Guid{});
    }

    // one batch by key name on the prospective copy, command by command against the oracle
    void update_by_key(const std::vector<Command>& script) {
        std::vector<janus::KeyCommand> cmds;
        std::vector<uint8_t> want_status, want_result;
        for (const Command& s : script) {
            janus::KeyCommand k;
            k.key = s.key;
            k.opId = s.op;
            k.arg = !s.has_arg ? 0 : s.arg.kind == oracle::Arg::Str ? 1 : s.arg.kind == oracle::Arg::Null ? 2 : 3;
            k.amount = s.arg.i;
            k.elem = s.arg.s;
            const auto it = sm.safeCRDTs.find(s.key);
            uint8_t st = JG_U_OK, res = 0;
            if (it == sm.safeCRDTs.end()) {
                st = JG_U_NO_KEY;
            } else {
                oracle::SafeCRDT& c = *it->second;
                oracle::GuidGen peek = *c.gen;  // the Guid.NewGuid() an Add will draw
                k.tag = G(peek.next());
                try {
                    res = c.Update(s.op, s.has_arg ? std::vector<oracle::Arg>{s.arg} : std::vector<oracle::Arg>{}, false).b ? 1 : 0;
                } catch (const oracle::InvalidOperationException&) {
                    st = JG_U_BAD_OP;
                } catch (const std::exception&) {  // the cast of args[0], or its absence
                    st = JG_U_BAD_ARG;
                }
            }
            cmds.push_back(k), want_status.push_back(st), want_result.push_back(res);
        }
        const std::vector<janus::KeyUpdate> got = janus::UpdateKeys(ks, prospective, cmds);
        for (size_t i = 0; i < script.size(); ++i) {
            const std::string at = "node " + std::to_string(id) + " command " + std::to_string(i) + " (" + script[i].key + ", op " + std::to_string(script[i].op) + ")";
            expect(got[i].status == want_status[i], at + ": status " + std::to_string(got[i].status) + ", the oracle says " + std::to_string(want_status[i]));
            expect(got[i].result == want_result[i], at + ": result");
            expect((got[i].idx == 0xFFFFFFFFu) == (got[i].status != JG_U_OK), at + ": idx");
        }
    }

    // SafeCRDT.Update on the oracle and the same op through the mirror's own path (ApplyOps)
    void update(const std::string& key, int op, const oracle::Arg& arg) {
        oracle::SafeCRDT& c = *sm.safeCRDTs.at(key);
        oracle::GuidGen peek = *c.gen;
        janus::ClientOp o;
        o.tag = G(peek.next());
        const bool want = c.Update(op, {arg}, false).b;
        o.uid = G(c.guid);
        o.opId = op;
        o.amount = arg.i;
        if (arg.kind == oracle::Arg::Str) o.elem = arg.s;
        expect((prospective.ApplyOps(std::vector<janus::ClientOp>{o})[0] != 0) == want, "ApplyOps on " + key + ": result");
    }
};

std::string member_of(const std::string& key) { return "m-" + key; }

// "gp" and "gs" of every key by name on one node against the oracle and, with `encoded`, the prospective copies' encoded
// states (compared while they hold this node's own writes only); returns how many answers of the two copies differ,
// the keys the script Clears or lowers left out
size_t read_all(Node& n, const std::vector<std::string>& keys, bool encoded) {
    std::vector<janus::KeyQuery> q;
    std::vector<std::vector<oracle::Arg>> args;
    for (const std::string& k : keys) {
        if (type_of(k) == janus::CrdtType::PNCounter) {
            q.push_back(janus::KeyQuery{k, false, std::nullopt});
            args.push_back({});
        } else {
            for (const auto& e : {std::optional<std::string>(member_of(k)), std::optional<std::string>("gone"), std::optional<std::string>("after"),
                                  std::optional<std::string>()}) {
                q.push_back(janus::KeyQuery{k, true, e});
                args.push_back({e ? oracle::Arg::S(*e) : oracle::Arg::N()});
            }
        }
    }
    const std::vector<janus::KeyAnswer> gp = janus::QueryKeys(n.ks, n.prospective, q), gs = janus::QueryKeys(n.ks, n.stable, q);
    size_t differ = 0;
    g_differing.clear();
    for (size_t i = 0; i < q.size(); ++i) {
        const oracle::SafeCRDT& c = *n.sm.safeCRDTs.at(q[i].key);
        const oracle::Result wp = c.QueryProspective(args[i]), ws = c.QueryStable(args[i]);
        const bool pnc = c.type == oracle::CrdtType::PNCounter;
        const std::string at = "node " + std::to_string(n.id) + " key " + q[i].key;
        expect(gp[i].status == JG_Q_OK && gs[i].status == JG_Q_OK, at + ": status");
        expect(gp[i].value == (pnc ? wp.i : (int64_t)wp.b), at + ": \"gp\" equals QueryProspective");
        expect(gs[i].value == (pnc ? ws.i : (int64_t)ws.b), at + ": \"gs\" equals QueryStable");
        // a Clear empties the prospective copy alone (the stable copy only ever merges, ORSet.cs:192-198 against
        // SafeCRDT.cs:80-83), and a negative Increment lowers a cell that the stable copy's max-merge of the earlier
        // snapshot keeps (PNCounters.cs:131-144): the two copies of those keys keep differing after the wave, in the
        // oracle too
        if (q[i].key != "orset3" && q[i].key != "orset5" && q[i].key != "pnc4" && gp[i].value != gs[i].value) ++differ, g_differing += " [" + at + "]";
    }
    if (!encoded) return differ;
    std::vector<janus::Guid> pu, ou;
    std::vector<std::string> pw, ow;
    for (const std::string& k : keys) {
        const oracle::SafeCRDT& c = *n.sm.safeCRDTs.at(k);
        if (c.type == oracle::CrdtType::PNCounter) pu.push_back(G(c.guid)), pw.push_back(oracle::json::EncodePNC(c.pncProspective->pnc.GetLastSynchronizedUpdate()));
        else ou.push_back(G(c.guid)), ow.push_back(oracle::json::EncodeORSet(c.orProspective->orset.GetLastSynchronizedUpdate()));
    }
    const std::vector<std::string> pg = n.prospective.EncodePNCStates(pu), og = n.prospective.EncodeORSetStates(ou);
    for (size_t i = 0; i < pu.size(); ++i) expect(pg[i] == pw[i], "node " + std::to_string(n.id) + ": PN-Counter state " + std::to_string(i) + "\n  got  " + pg[i] + "\n  want " + pw[i]);
    for (size_t i = 0; i < ou.size(); ++i) expect(og[i] == ow[i], "node " + std::to_string(n.id) + ": OR-Set state " + std::to_string(i) + "\n  got  " + og[i] + "\n  want " + ow[i]);
    return differ;
}

std::vector<janus::UpdateMessage> blocks_of(const oracle::SafeCRDTManager& sm) {
    std::vector<janus::UpdateMessage> block;
    for (const oracle::UpdateMessage& um : sm.submitted) {
        janus::UpdateMessage b;
        for (const oracle::NetworkProtocol& np : um.update) {
            janus::NetworkProtocol m;
            m.uid = G(np.uid);
            m.message = np.bytes;
            b.update.push_back(m);
        }
        block.push_back(b);
    }
    return block;
}

void FourNodeWritesByName() {
    using A = oracle::Arg;
    std::vector<std::unique_ptr<Node>> node;
    for (int i = 0; i < 4; ++i) node.emplace_back(new Node(i));
    std::vector<std::string> keys;
    for (uint64_t k = 0; k < 12; ++k) {
        keys.push_back((k % 2 ? "orset" : "pnc") + std::to_string(k));
        const jg_guid g{0x2000 + k, 0xFEDCBA0000000000ull + k * 31};
        expect(node[0]->ks.CreateNewKVPair(keys.back(), g), "CreateNewKVPair");
        node[0]->create_crdt(keys.back(), g);
    }
    const std::vector<std::string> states{node[0]->ks.Encode()};
    for (int i = 1; i < 4; ++i)
        expect(node[i]->ks.Receive(states, [&](const std::string& k, const jg_guid& g) { node[i]->create_crdt(k, g); }) == -1, "Receive");

    // the scripted commands, one batch per node
    for (int i = 0; i < 4; ++i) {
        std::vector<Command> s;
        for (size_t k = 0; k < keys.size(); ++k) {
            const std::string& key = keys[k];
            if (type_of(key) == janus::CrdtType::PNCounter) {
                s.push_back({key, 1, true, A::I(10 + 3 * (int)k + i)});
                if ((k + i) % 3 == 0) s.push_back({key, 2, true, A::I(1 + i)});
                if (k == 4) s.push_back({key, 1, true, A::I(-7)});
            } else {
                if ((k + i) % 2 == 0) s.push_back({key, 1, true, A::S(member_of(key))});
                s.push_back({key, 1, true, A::S("gone")});
                if (i == 1) s.push_back({key, 2, true, A::S("gone")});
                if (k % 3 == 0 && i == 2) s.push_back({key, 1, true, A::N()});
                if (k == 5 && i >= 2) s.push_back({key, 3, false, A::N()}), s.push_back({key, 1, true, A::S("after")});
                if (k == 7) s.push_back({key, 2, true, A::S("never added")}), s.push_back({key, 2, true, A::N()});
            }
        }
        s.push_back({"absent", 1, true, A::I(1)});     // an unknown key
        s.push_back({"pnc0", 1, true, A::S("x")});     // arguments of the wrong type
        s.push_back({"pnc0", 2, true, A::N()});
        s.push_back({"orset1", 1, true, A::I(5)});
        s.push_back({"pnc2", 1, false, A::N()});       // no argument
        s.push_back({"orset1", 2, false, A::N()});
        s.push_back({"pnc0", 3, true, A::I(1)});       // operation ids no wrapper knows
        s.push_back({"pnc0", 3, false, A::N()});       // (the cast comes first: a bad argument)
        s.push_back({"orset1", 4, true, A::S("x")});
        s.push_back({"orset1", 0, false, A::N()});
        s.push_back({"orset3", 3, true, A::I(9)});     // Clear reads no argument
        s.push_back({"orset3", 1, true, A::S("after")});
        Node& n = *node[i];
        n.update_by_key(s);
        expect(read_all(n, keys, true) > 0, "\"gs\" stays as it was until a committed wave");
        // the mirror's own path (ApplyOps) on sets the batch Cleared and on names it interned, a second batch by key
        // behind names the mirror interned, and the mirror's path once more
        n.update("orset5", 1, A::S("after"));
        n.update("orset5", 1, A::S("post"));
        n.update("orset3", 2, A::S("after"));
        n.update("orset3", 1, A::S("gone"));
        n.update("pnc0", 1, A::I(3));
        n.update_by_key({{"orset5", 2, true, A::S("post")}, {"orset3", 1, true, A::S("post")}, {"orset5", 3, false, A::N()}, {"orset5", 1, true, A::S("post")},
                         {"pnc0", 2, true, A::I(2)}});
        n.update("orset5", 1, A::S("last"));
        expect(read_all(n, keys, true) > 0, "\"gs\" stays as it was until a committed wave");
    }
    // every node's blocks reach the other nodes' prospective copies (ReceivedBlock; RM:290-344)
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            if (i == j) continue;
            for (const oracle::UpdateMessage& um : node[j]->sm.submitted)
                for (const oracle::NetworkProtocol& np : um.update) {
                    oracle::SafeCRDT& c = *node[i]->sm.safeCRDTsIndexedByuid.at(np.uid);
                    if (c.type == oracle::CrdtType::PNCounter) c.pncProspective->pnc.Merge(oracle::json::DecodePNC<int32_t>(np.bytes));
                    else c.orProspective->orset.Merge(oracle::json::DecodeORSet(np.bytes));
                }
            node[i]->prospective.ReceivedBlock(blocks_of(node[j]->sm));
        }
    // one committed wave: every node's submitted messages, in node order, to every stable copy
    std::vector<std::vector<janus::UpdateMessage>> wave(1);
    std::vector<std::vector<oracle::UpdateMessage>> owave(1);
    for (int j = 0; j < 4; ++j) {
        for (const oracle::UpdateMessage& um : node[j]->sm.submitted) owave[0].push_back(um);
        for (const janus::UpdateMessage& b : blocks_of(node[j]->sm)) wave[0].push_back(b);
    }
    for (int i = 0; i < 4; ++i) {
        node[i]->stable.ApplyCommitted(wave);
        node[i]->sm.HandleAfterConsensusUpdates(owave);
        expect(read_all(*node[i], keys, false) == 0, "after the wave \"gs\" and \"gp\" agree:" + g_differing);
    }
}

}  // namespace

int main() {
    check(jg_open(0, &g_ctx), "jg_open");
    const std::vector<std::pair<std::string, std::function<void()>>> tests = {{"Update.FourNodeWritesByName", FourNodeWritesByName}};
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
