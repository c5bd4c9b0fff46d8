// host/kat_adopt.cpp — kat_keyspace's four nodes without type_of(key) and without any host row map: the node
// allocates every row and set id (csrc/adopt.hip).  Node 0 creates PN-Counter and OR-Set keys with jg_node_create_uids
// on both copies plus jg_keyspace_create_keys and ships the ManagerMsg_Create messages and the key-space state; the
// other nodes run jg_node_create_uids on the prospective copy (ReplicationManager.ReceivedNewObjectSyncMsg),
// jg_keyspace_receive, then jg_node_adopt_keys (OnNext's CreateSafeCRDT).  One key's Create message arrives late: its
// record is JG_A_NO_TYPE until the uid is created and the range adopted again.  Every node then applies one committed
// wave and answers "gp" / "gs" for every key by name, checked against the oracle's SafeCRDTManager and, for the learnt
// keys, host/tpset_ref.hpp's OnNext.  Prints "PASS name" / "FAIL name: why"; exit 0 = every scenario passes.
#include <cstdio>
#include <functional>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "janus_gpu.h"
#include "json.hpp"
#include "oracle.hpp"
#include "tpset_ref.hpp"

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

struct Create {  // NetworkProtocol{uid, ManagerMsg_Create, type}: what ReceivedNewObjectSyncMsg reads
    jg_guid uid;
    uint8_t type;  // 0 PNCounter, 1 ORSet: the caller's mapping of NetworkProtocol.type
};

struct Copy {  // one copy of a node's keys: its stores and its jg_node; no map, no allocator
    jg_pnc* pnc = nullptr;
    jg_orset* orset = nullptr;
    jg_node* node = nullptr;
    jg_guid replica;
    explicit Copy(jg_guid r) : replica(r) {
        check(jg_pnc_create(g_ctx, 2, 4, 4, &pnc), "jg_pnc_create");  // two rows: the store grows as keys arrive
        check(jg_orset_create(g_ctx, 0, 0, &orset), "jg_orset_create");
        check(jg_node_create(pnc, orset, &node), "jg_node_create");
    }
    ~Copy() {
        (void)jg_node_destroy(node);
        (void)jg_orset_destroy(orset);
        (void)jg_pnc_destroy(pnc);
    }
    std::vector<uint8_t> create(const std::vector<Create>& c) {
        std::vector<jg_guid> uid, rep(c.size(), replica);
        std::vector<uint8_t> type, status(c.size() + 1);
        for (const Create& x : c) uid.push_back(x.uid), type.push_back(x.type);
        check(jg_node_create_uids(node, c.size(), uid.data(), type.data(), rep.data(), 256, status.data(), nullptr), "jg_node_create_uids");
        status.resize(c.size());
        return status;
    }
};

struct Node {
    int id;
    jg_keyspace* ks = nullptr;
    janus::ref::KeySpace ref;
    Copy stable, prospective;
    oracle::SafeCRDTManager sm;
    std::map<std::pair<uint64_t, uint64_t>, uint8_t> rm_types;  // the oracle side's ReplicationManager.GetCRDTType
    uint64_t adopted_to = 0;
    explicit Node(int i)
        : id(i), stable(jg_guid{0x57AB1E00ull + (uint64_t)i, 1}), prospective(jg_guid{0x9405900ull + (uint64_t)i, 2}), sm(1, 0x9000 + (uint64_t)i) {
        check(jg_keyspace_create(g_ctx, 256, 1 << 16, &ks), "jg_keyspace_create");
    }
    ~Node() { (void)jg_keyspace_destroy(ks); }

    // CreateCRDTInstance on the creating node: both copies, the dictionary, the oracle's SafeCRDT
    void create_local(const std::string& key, const Create& c) {
        expect(stable.create({c})[0] == JG_C_CREATED && prospective.create({c})[0] == JG_C_CREATED, "a new uid is created on both copies");
        const uint64_t off[2] = {0, key.size()};
        uint8_t added = 0;
        check(jg_keyspace_create_keys(ks, 1, off, reinterpret_cast<const uint8_t*>(key.data()), &c.uid, &added), "jg_keyspace_create_keys");
        expect(added == 1 && ref.CreateNewKVPair(key, oracle::Guid{c.uid.lo, c.uid.hi}), "CreateNewKVPair's TryAdd");
        sm.CreateSafeCRDT(key, c.type ? oracle::CrdtType::ORSet : oracle::CrdtType::PNCounter, oracle::Guid{c.uid.lo, c.uid.hi});
    }
    // ReceivedNewObjectSyncMsg for a batch of ManagerMsg_Create
    void receive_creates(const std::vector<Create>& c, uint8_t want) {
        for (uint8_t s : prospective.create(c)) expect(s == want, "jg_node_create_uids' status on the prospective copy");
        for (const Create& x : c) rm_types[{x.uid.lo, x.uid.hi}] = x.type;
    }
    std::string encode_keyspace() {
        jg_tpset* set = nullptr;
        check(jg_keyspace_set(ks, &set), "jg_keyspace_set");
        uint64_t nb = 0;
        check(jg_tpset_encode_json(set, &nb, nullptr, 0), "jg_tpset_encode_json (size)");
        std::string out(nb, '\0');
        check(jg_tpset_encode_json(set, &nb, reinterpret_cast<uint8_t*>(out.data()), nb), "jg_tpset_encode_json");
        return out;
    }
    void receive_state(const std::string& state) {
        const uint64_t off[2] = {0, state.size()};
        uint64_t n_new = 0;
        check(jg_keyspace_receive(ks, 1, off, reinterpret_cast<const uint8_t*>(state.data()), 0, nullptr, nullptr, &n_new), "jg_keyspace_receive");
        const size_t before = ref.journal().size();
        expect(ref.Receive(state) == 0 && ref.journal().size() - before == n_new, "the journal grows as the restatement's");
    }
    // OnNext's CreateSafeCRDT over the journal from `from`: statuses against the restatement's records and the
    // oracle side's GetCRDTType; the oracle's SafeCRDT for every record adopted
    void adopt(uint64_t from) {
        uint64_t to = 0, nb = 0;
        check(jg_keyspace_new_keys(ks, from, &to, &nb, nullptr, nullptr, nullptr, nullptr), "jg_keyspace_new_keys (size)");
        expect(to == ref.journal().size(), "the journal's length");
        const uint64_t n = to - from;
        std::vector<jg_guid> rep(n + 1, stable.replica);
        std::vector<uint8_t> status(n + 1), kind(n + 1);
        std::vector<uint32_t> idx(n + 1);
        check(jg_node_adopt_keys(stable.node, prospective.node, ks, from, to, rep.data(), 256, status.data(), kind.data(), idx.data()), "jg_node_adopt_keys");
        for (uint64_t j = from; j < to; ++j) {
            const auto& r = ref.journal()[j];
            const auto t = rm_types.find({r.guid.lo, r.guid.hi});
            const bool held = sm.safeCRDTsIndexedByuid.count(r.guid) != 0;
            const uint8_t want = r.status != 0 ? JG_A_SKIPPED : t == rm_types.end() ? JG_A_NO_TYPE : held ? JG_A_HAVE : JG_A_ADOPTED;
            expect(status[j - from] == want, "node " + std::to_string(id) + " record " + std::to_string(j) + ": jg_node_adopt_keys' status");
            if (want == JG_A_ADOPTED || want == JG_A_HAVE) expect(kind[j - from] == t->second, "the kind is the Create message's");
            if (want == JG_A_ADOPTED) sm.CreateSafeCRDT(r.bytes, t->second ? oracle::CrdtType::ORSet : oracle::CrdtType::PNCounter, r.guid);
        }
        adopted_to = to;
    }
};

struct Answer { int64_t value; uint8_t status, kind; };
std::vector<Answer> query(Node& n, jg_node* copy, const std::vector<std::string>& keys, const std::vector<oracle::Arg>& args) {
    std::string kb, eb;
    std::vector<uint64_t> koff{0}, eoff{0};
    std::vector<uint8_t> flag;
    for (size_t i = 0; i < keys.size(); ++i) {
        kb += keys[i], koff.push_back(kb.size());
        if (args[i].kind == oracle::Arg::Str) eb += args[i].s;
        eoff.push_back(eb.size());
        flag.push_back(args[i].kind == oracle::Arg::Str ? 1 : args[i].kind == oracle::Arg::Null ? 2 : 0);
    }
    std::vector<int64_t> value(keys.size());
    std::vector<uint8_t> status(keys.size()), kind(keys.size());
    eb += '\0';
    check(jg_node_query_keys(copy, n.ks, keys.size(), koff.data(), reinterpret_cast<const uint8_t*>(kb.data()), eoff.data(),
                             reinterpret_cast<const uint8_t*>(eb.data()), flag.data(), value.data(), status.data(), kind.data(), nullptr),
          "jg_node_query_keys");
    std::vector<Answer> out;
    for (size_t i = 0; i < keys.size(); ++i) out.push_back(Answer{value[i], status[i], kind[i]});
    return out;
}

void FourNodeCreateAdoptAndApply() {
    std::vector<std::unique_ptr<Node>> node;
    for (int i = 0; i < 4; ++i) node.emplace_back(new Node(i));
    std::vector<std::pair<std::string, Create>> made;
    for (uint64_t k = 0; k < 20; ++k)
        made.push_back({"key" + std::to_string(k), Create{jg_guid{0x3000 + k, 0xABCDEF0000000000ull + k * 77}, (uint8_t)((k * 7 / 3) % 2)}});
    const auto own = std::make_pair(std::string("key4"), Create{jg_guid{7, 7}, 1});
    node[2]->create_local(own.first, own.second);  // node 2 made key4 itself first, an ORSet under its own guid
    std::vector<Create> creates;
    for (const auto& m : made) node[0]->create_local(m.first, m.second), creates.push_back(m.second);
    uint32_t row = 0, set = 0;
    check(jg_node_next_idx(node[0]->stable.node, &row, &set), "jg_node_next_idx");
    expect(row + set == made.size() && row > 2, "every key took the next row or set id of its kind; the store grew");
    const std::string state = node[0]->encode_keyspace();
    const std::vector<Create> early(creates.begin(), creates.end() - 1), late(creates.end() - 1, creates.end());
    for (int i = 1; i < 4; ++i) {
        Node& n = *node[i];
        n.receive_creates(early, JG_C_CREATED);
        n.receive_state(state);
        n.adopt(0);  // the last key's Create message has not arrived: NO_TYPE
        n.receive_creates(early, JG_C_EXISTS);  // a Create received again: the first creation stands
        n.receive_creates(late, JG_C_CREATED);
        n.adopt(0);  // the same range again: HAVE everywhere but the late key
        n.receive_state(state);  // a state received again journals nothing
        n.adopt(n.adopted_to);
    }

    // one committed wave: a state for every uid node 0 made, from a replica none of the four is
    std::vector<jg_guid> uid;
    std::vector<uint8_t> type;
    std::vector<uint64_t> off{0};
    std::string bytes;
    std::vector<std::vector<oracle::UpdateMessage>> owave(1);
    owave[0].emplace_back();
    for (uint64_t k = 0; k < made.size(); ++k) {
        std::string b;
        if (made[k].second.type == 0) {
            oracle::PNCounter<int32_t> src(oracle::Guid{0xABC000 + k, 0x51C});
            src.Increment((int32_t)(10 + 3 * k));
            src.Decrement((int32_t)(k % 4));
            b = oracle::json::EncodePNC(src.GetLastSynchronizedUpdate());
        } else {
            oracle::ORSet src;
            src.AddTag(std::string("e") + std::to_string(k), oracle::Guid{0x7A6000 + k, 1});
            src.AddTag(std::string("gone\"\\"), oracle::Guid{0x7A6000 + k, 2});
            src.Remove(std::string("gone\"\\"));
            if (k % 3 == 0) src.AddTag(std::nullopt, oracle::Guid{0x7A6000 + k, 3});
            b = oracle::json::EncodeORSet(src.GetLastSynchronizedUpdate());
        }
        uid.push_back(made[k].second.uid), type.push_back(1), bytes += b, off.push_back(bytes.size());
        oracle::NetworkProtocol np;
        np.uid = oracle::Guid{made[k].second.uid.lo, made[k].second.uid.hi};
        np.bytes = b;
        owave[0][0].update.push_back(np);
    }
    const jg_commit wave{uid.size(), uid.data(), type.data(), nullptr, off.data(), reinterpret_cast<const uint8_t*>(bytes.data()), nullptr, nullptr};
    for (int i = 0; i < 4; ++i) {
        Node& n = *node[i];
        uint64_t at = 0;
        check(jg_apply_committed(n.stable.node, nullptr, &wave, nullptr, nullptr, &at), "jg_apply_committed");
        expect(at == UINT64_MAX, "the wave applies whole");
        n.sm.HandleAfterConsensusUpdates(owave);
        std::vector<std::string> keys;
        std::vector<oracle::Arg> args;
        for (uint64_t k = 0; k < made.size(); ++k) {
            const oracle::SafeCRDT& c = *n.sm.safeCRDTs.at(made[k].first);
            if (c.type == oracle::CrdtType::PNCounter) {
                keys.push_back(made[k].first), args.push_back(oracle::Arg::I(0));  // an Int stands for "no argument" (flag 0)
            } else {
                for (const oracle::Arg& a : {oracle::Arg::S("e" + std::to_string(k)), oracle::Arg::S("gone\"\\"), oracle::Arg::N(), oracle::Arg::S("never")})
                    keys.push_back(made[k].first), args.push_back(a);
            }
        }
        const std::vector<Answer> gs = query(n, n.stable.node, keys, args), gp = query(n, n.prospective.node, keys, args);
        for (size_t q = 0; q < keys.size(); ++q) {
            const oracle::SafeCRDT& c = *n.sm.safeCRDTs.at(keys[q]);
            const bool pnc = c.type == oracle::CrdtType::PNCounter;
            const std::vector<oracle::Arg> a = pnc ? std::vector<oracle::Arg>{} : std::vector<oracle::Arg>{args[q]};
            const oracle::Result ws = c.QueryStable(a), wp = c.QueryProspective(a);
            const std::string where = "node " + std::to_string(i) + " key " + keys[q];
            expect(gs[q].status == JG_Q_OK && gp[q].status == JG_Q_OK, where + ": status");
            expect(gs[q].kind == (pnc ? 0 : 1) && gp[q].kind == gs[q].kind, where + ": kind");
            expect(gs[q].value == (pnc ? ws.i : (int64_t)ws.b), where + ": \"gs\" equals QueryStable");
            expect(gp[q].value == (pnc ? wp.i : (int64_t)wp.b), where + ": \"gp\" equals QueryProspective");
        }
    }
    // node 2 keeps key4 under its own guid (the dictionary held the key: nothing was journalled, nothing adopted), and its
    // stable copy skipped the wave's state for node 0's key4
    expect(node[2]->sm.safeCRDTs.at("key4")->guid == (oracle::Guid{7, 7}), "key4 on node 2");
}

}  // namespace

int main() {
    check(jg_open(0, &g_ctx), "jg_open");
    const std::vector<std::pair<std::string, std::function<void()>>> tests = {{"Adopt.FourNodeCreateAdoptAndApply", FourNodeCreateAdoptAndApply}};
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
