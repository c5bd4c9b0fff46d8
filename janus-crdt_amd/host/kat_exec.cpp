// host/kat_exec.cpp — a client stream with its "gp" reads in order among the writes (jg_node_exec_keys) on the
// device against the oracle's SafeCRDT.Update (BFT-CRDT/SafeCRDTs/SafeCRDT.cs:39-62) and SafeCRDT.QueryProspective
// (SafeCRDT.cs:64-78) run one by one, on kat_update_ship's four nodes.  Every node takes kat_update_ship's two scripted
// batches BY KEY NAME on its prospective copy (janus::GpuStableStore::ExecKeys, one jg_node_exec_keys each) with a read
// of the same key behind every command but the last: a counter's Get, a set's Contains of "m", "gone", the null element
// or of nothing (ORSetWrapper.Query dereferences args[0]), and a read of a key nobody created.
//   safe      every write a safe update (snap 1): every applied write's bytes and SHA-256 are held to the message the
//             oracle's SafeCRDT.Update submitted for it; every read's status and value to QueryProspective at that point;
//   batched   after every node's blocks reached the other prospective copies, every write non-safe (snap 2) and the
//             oracle's batcher flushing once at the end: the writes that ship are exactly the objects it kept.
// Then "gp" / "gs" of every key are the oracle's, before and after a committed wave.  Prints "PASS name" / "FAIL name: why".
#include <cstdio>
#include <functional>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "digest.hpp"
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

janus::Guid G(const oracle::Guid& g) { return janus::Guid{g.lo, g.hi}; }
bool is_pnc(const std::string& key) { return key.compare(0, 3, "pnc") == 0; }

struct Command {
    std::string key;
    int op;
    bool has_arg;
    oracle::Arg arg;
    bool read = false;
};

struct Node {
    int id;
    janus::GpuKeySpace ks;
    janus::GpuStableStore stable, prospective;
    oracle::SafeCRDTManager sm;
    explicit Node(int i) : id(i), ks(g_ctx, 256, 1 << 16), stable(g_ctx, 256, 8, 4), prospective(g_ctx, 256, 8, 4), sm(1, 0xA000 + (uint64_t)i) {}

    // the oracle's CRDT first: the device copies take its replica Guids, so the encoded states can be compared
    void create_crdt(const std::string& key, const jg_guid& g) {
        const janus::CrdtType t = is_pnc(key) ? janus::CrdtType::PNCounter : janus::CrdtType::ORSet;
        oracle::SafeCRDT& c = sm.CreateSafeCRDT(key, is_pnc(key) ? oracle::CrdtType::PNCounter : oracle::CrdtType::ORSet, oracle::Guid{g.lo, g.hi});
        const janus::Guid uid{g.lo, g.hi};
        stable.CreateSafeCRDT(uid, t, is_pnc(key) ? G(c.pncStable->pnc.replicaIdx()) : janus::Guid{});
        prospective.CreateSafeCRDT(uid, t, is_pnc(key) ? G(c.pncProspective->pnc.replicaIdx()) : janus::Guid{});
    }

    // One batch: the oracle command by command (safe: each Update submits its own message; else one flush at the end), then
    // the same batch in one call.  The script's last command is an applied PN-Counter command (it triggers the flush).
    void batch(const std::vector<Command>& script, bool safe) {
        const size_t n = script.size();
        std::vector<janus::KeyCommand> cmds;
        std::vector<uint8_t> want_status(n, JG_U_OK), want_result(n, 0);
        std::vector<int64_t> want_value(n, 0);
        std::vector<std::string> sent(n);  // safe: SafeCRDT.Update's message of command i
        const size_t first = sm.submitted.size();
        sm.clientBatchSize = safe ? 1 : 1 << 30;
        for (size_t i = 0; i < n; ++i) {
            const Command& s = script[i];
            janus::KeyCommand k;
            k.key = s.key;
            k.opId = s.op;
            k.arg = !s.has_arg ? 0 : s.arg.kind == oracle::Arg::Str ? 1 : s.arg.kind == oracle::Arg::Null ? 2 : 3;
            k.amount = s.arg.i;
            k.elem = s.arg.s;
            k.read = s.read;
            const auto it = sm.safeCRDTs.find(s.key);
            if (it == sm.safeCRDTs.end()) {
                want_status[i] = s.read ? JG_Q_NO_KEY : JG_U_NO_KEY;
            } else if (s.read) {  // SafeCRDT.QueryProspective at this point of the stream
                const oracle::SafeCRDT& c = *it->second;
                try {
                    const oracle::Result r = c.QueryProspective(s.has_arg ? std::vector<oracle::Arg>{s.arg} : std::vector<oracle::Arg>{});
                    want_value[i] = c.type == oracle::CrdtType::PNCounter ? r.i : (int64_t)r.b;
                } catch (const oracle::OverflowException&) {
                    want_status[i] = JG_Q_OVERFLOW;
                } catch (const std::exception&) {
                    want_status[i] = JG_Q_NO_ARG;
                }
            } else {
                oracle::SafeCRDT& c = *it->second;
                oracle::GuidGen peek = *c.gen;  // the Guid.NewGuid() an Add will draw
                k.tag = G(peek.next());
                if (!safe && i + 1 == n) sm.clientBatchSize = (int)sm.clientUpdateBuffer.size() + 1;  // this Update flushes the batch
                const size_t before = sm.submitted.size();
                try {
                    want_result[i] = c.Update(s.op, s.has_arg ? std::vector<oracle::Arg>{s.arg} : std::vector<oracle::Arg>{}, safe, 1 + (uint64_t)id).b ? 1 : 0;
                    if (safe) {
                        expect(sm.submitted.size() == before + 1 && sm.submitted.back().update.size() == 1, "the oracle's batcher submits a safe update on its own");
                        sent[i] = sm.submitted.back().update[0].bytes;
                    }
                } catch (const oracle::InvalidOperationException&) {
                    want_status[i] = JG_U_BAD_OP;
                } catch (const std::exception&) {
                    want_status[i] = JG_U_BAD_ARG;
                }
            }
            cmds.push_back(k);
        }
        std::vector<janus::KeyMessage> msg;
        uint32_t rounds = 0;
        const std::vector<janus::KeyUpdate> got = prospective.ExecKeys(ks, cmds, std::vector<uint8_t>(n, safe ? 1 : 2), msg, &rounds);
        expect(safe ? rounds >= 3 : rounds == 1, "node " + std::to_string(id) + ": " + std::to_string(rounds) + " rounds");
        const std::string nd = "node " + std::to_string(id) + (safe ? " safe" : " batched") + " command ";
        std::map<std::string, size_t> shipped;  // batched: key -> the command that shipped its object's state
        for (size_t i = 0; i < n; ++i) {
            const std::string at = nd + std::to_string(i) + " (" + script[i].key + ", op " + std::to_string(script[i].op) + ")";
            expect(got[i].status == want_status[i], at + ": status " + std::to_string(got[i].status) + ", the oracle says " + std::to_string(want_status[i]));
            expect(got[i].result == want_result[i], at + ": result");
            expect(got[i].value == want_value[i], at + ": value " + std::to_string(got[i].value) + ", the oracle says " + std::to_string(want_value[i]));
            const bool applied = got[i].status == JG_U_OK && !script[i].read;
            if (!applied || (!safe && msg[i].message.empty())) {
                expect(msg[i].message.empty(), at + ": a command that ships no snapshot has bytes");
                expect(msg[i].sha256 == std::array<uint8_t, 32>{}, at + ": its hash is not zero");
                continue;
            }
            if (safe) expect(msg[i].message == sent[i], at + ": message\n  got  " + msg[i].message + "\n  want " + sent[i]);
            else expect(shipped.emplace(script[i].key, i).second, at + ": two states of one object survived");
            std::array<uint8_t, 32> h;
            oracle::sha256(reinterpret_cast<const uint8_t*>(msg[i].message.data()), msg[i].message.size(), h.data());
            expect(msg[i].sha256 == h, at + ": SHA-256");
        }
        if (safe) return;
        // what ActualPropagateSyncMsg kept for the batch: one message per object, its latest
        expect(sm.submitted.size() == first + 1, nd + "(end): the oracle's batcher flushed once");
        size_t kept = 0;
        for (const oracle::NetworkProtocol& np : sm.submitted.back().update) {
            const oracle::SafeCRDT& c = *sm.safeCRDTsIndexedByuid.at(np.uid);
            ++kept;
            const auto it = shipped.find(c.key);
            expect(it != shipped.end(), nd + "(end): the batcher kept " + c.key + ", the call shipped nothing for it");
            expect(msg[it->second].message == np.bytes, nd + std::to_string(it->second) + " (" + c.key + "): the state the batcher kept\n  got  " +
                                                            msg[it->second].message + "\n  want " + np.bytes);
            size_t last = 0;
            for (size_t i = 0; i < n; ++i)
                if (script[i].key == c.key && got[i].status == JG_U_OK && !script[i].read) last = i;
            expect(it->second == last, nd + "(end): the survivor of " + c.key + " is its last applied command");
        }
        expect(kept == shipped.size(), nd + "(end): the call shipped objects the batcher did not keep");
    }
};

// "gp" and "gs" of every key by name against the oracle
void read_all(Node& n, const std::vector<std::string>& keys) {
    std::vector<janus::KeyQuery> q;
    std::vector<std::vector<oracle::Arg>> args;
    for (const std::string& k : keys) {
        if (is_pnc(k)) {
            q.push_back(janus::KeyQuery{k, false, std::nullopt});
            args.push_back({});
        } else {
            for (const char* e : {"m", "gone"}) {
                q.push_back(janus::KeyQuery{k, true, std::string(e)});
                args.push_back({oracle::Arg::S(e)});
            }
        }
    }
    const std::vector<janus::KeyAnswer> gp = janus::QueryKeys(n.ks, n.prospective, q), gs = janus::QueryKeys(n.ks, n.stable, q);
    for (size_t i = 0; i < q.size(); ++i) {
        const oracle::SafeCRDT& c = *n.sm.safeCRDTs.at(q[i].key);
        const bool pnc = c.type == oracle::CrdtType::PNCounter;
        const std::string at = "node " + std::to_string(n.id) + " key " + q[i].key;
        // The stable copy max-merges every shipped snapshot, also the one from before the cell wrapped: after the wave
        // the checked Sum of those cells overflows in the oracle, and the device reports the same.
        const auto same = [&](const janus::KeyAnswer& got, bool prospective, const char* what) {
            try {
                const oracle::Result want = prospective ? c.QueryProspective(args[i]) : c.QueryStable(args[i]);
                expect(got.status == JG_Q_OK, at + ": status of " + what);
                expect(got.value == (pnc ? want.i : (int64_t)want.b), at + ": " + what + " equals the oracle's");
            } catch (const oracle::OverflowException&) {
                expect(got.status == JG_Q_OVERFLOW, at + ": the oracle's " + what + " overflows, the device's does not");
            }
        };
        same(gp[i], true, "\"gp\"");
        same(gs[i], false, "\"gs\"");
    }
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

std::vector<Command> script_of(const std::vector<std::string>& keys, int i, int round) {
    using A = oracle::Arg;
    std::vector<Command> s;
    s.push_back({"orset5", 3, false, A::I(0)});                                             // cleared with nothing shipped before
    s.push_back({"orset1", 1, true, A::S("early")}), s.push_back({"orset1", 3, false, A::I(0)});  // cleared after a shipped command
    s.push_back({"orset3", 1, true, A::S("twice")}), s.push_back({"orset3", 3, false, A::I(0)}), s.push_back({"orset3", 3, true, A::S("ignored")});
    for (int rep = 0; rep < 3; ++rep)
        for (size_t k = 0; k < keys.size(); ++k) {
            const std::string& key = keys[k];
            if (is_pnc(key)) {
                s.push_back({key, 1, true, A::I(10 + 3 * (int)k + i + 100 * rep)});
                if ((k + i + rep) % 3 == 0) s.push_back({key, 2, true, A::I(1 + i)});
                if (k == 4) s.push_back({key, 1, true, A::I(-7 - round)});
                if (k == 2 && rep == 1) s.push_back({key, 1, true, A::I(2147483000)}), s.push_back({key, 1, true, A::I(2147483000)});  // wraps an int
            } else {
                if ((k + i + rep) % 2 == 0) s.push_back({key, 1, true, A::S("m")});
                if (rep == 2) s.push_back({key, 1, true, A::S("gone")}), s.push_back({key, 2, true, A::S("gone")});
                if ((k + i) % 4 == 1 && rep == 1) s.push_back({key, 3, false, A::I(0)}), s.push_back({key, 2, true, A::S("never there")});
                if (k == 7) s.push_back({key, 1, true, A::N()});
            }
            if (k == 3) s.push_back({"absent", 1, true, A::I(1)});       // failed commands between a row's commands
            if (k == 6) s.push_back({"pnc0", 1, true, A::S("x")});
            if (k == 8) s.push_back({"pnc0", 3, true, A::I(1)}), s.push_back({"orset1", 1, true, A::I(5)});
        }
    for (int h = 0; h < 70; ++h) s.push_back({h % 2 ? "pnc6" : "pnc0", h % 5 == 0 ? 2 : 1, true, A::I(h - 20)});  // two hot rows, more than a wave
    // a read of the same key behind every command: Get for a counter (any argument is ignored), for a set Contains of
    // "m", "gone", the null element, or of nothing; then the last command, which applies (the batched round's flush)
    std::vector<Command> out;
    for (size_t j = 0; j < s.size(); ++j) {
        out.push_back(s[j]);
        Command r{s[j].key, 0, true, A::S(j % 2 ? "m" : "gone"), true};
        if (is_pnc(s[j].key) && j % 3 == 0) r.has_arg = false;
        if (!is_pnc(s[j].key) && j % 7 == 3) r.arg = A::N();
        if (!is_pnc(s[j].key) && j % 11 == 5) r.has_arg = false;
        out.push_back(r);
    }
    out.push_back({"pnc10", 1, true, A::I(1)});
    return out;
}

void FourNodeWritesThatShip() {
    std::vector<std::unique_ptr<Node>> node;
    for (int i = 0; i < 4; ++i) node.emplace_back(new Node(i));
    std::vector<std::string> keys;
    for (uint64_t k = 0; k < 12; ++k) {
        keys.push_back((k % 2 ? "orset" : "pnc") + std::to_string(k));
        const jg_guid g{0x3000 + k, 0xFEDCBA0000000000ull + k * 37};
        expect(node[0]->ks.CreateNewKVPair(keys.back(), g), "CreateNewKVPair");
        node[0]->create_crdt(keys.back(), g);
    }
    const std::vector<std::string> states{node[0]->ks.Encode()};
    for (int i = 1; i < 4; ++i)
        expect(node[i]->ks.Receive(states, [&](const std::string& k, const jg_guid& g) { node[i]->create_crdt(k, g); }) == -1, "Receive");

    for (int i = 0; i < 4; ++i) {
        node[i]->batch(script_of(keys, i, 0), true);
        read_all(*node[i], keys);
    }
    // every node's blocks reach the other nodes' prospective copies (ReceivedBlock): rows of several replicas
    std::vector<size_t> sent(4);
    for (int j = 0; j < 4; ++j) sent[j] = node[j]->sm.submitted.size();
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
    for (int i = 0; i < 4; ++i) {
        node[i]->batch(script_of(keys, i, 1), false);
        read_all(*node[i], keys);
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
        read_all(*node[i], keys);
    }
}

}  // namespace

int main() {
    check(jg_open(0, &g_ctx), "jg_open");
    const std::vector<std::pair<std::string, std::function<void()>>> tests = {{"Exec.FourNodeStreamsWithReadsInOrder", FourNodeWritesThatShip}};
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
