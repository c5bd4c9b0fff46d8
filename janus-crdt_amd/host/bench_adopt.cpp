// host/bench_adopt.cpp — a joining node turns learnt keys into CRDTs (csrc/adopt.hip) beside the
// parent's way.  Node 0's key-space state holds K keys, half PN-Counter, half OR-Set, and its K ManagerMsg_Create
// messages name each uid's type.  A run starts from an empty node (key space, both copies) and is
//   device way    jg_keyspace_receive; jg_node_create_uids on the prospective copy; jg_node_adopt_keys on the stable one
//   parent's way  jg_keyspace_receive; the Create messages into a host uid -> type map and a host row allocator ->
//                 jg_node_register + jg_pnc_intern on the prospective copy; jg_keyspace_new_keys readback -> the map ->
//                 the allocator -> jg_node_register + jg_pnc_intern on the stable copy
//   (1) K = 1,000,000    (2) K = 10,000
// Wall time of the calls a caller makes, receive included; the two ways alternate, the parent's way twice per repetition:
// the distance of its two medians is the A/A spread a difference has to exceed.  Every repetition compares the two ways'
// indices record by record, both nodes' allocation marks, every key's kind and status by name on both copies and every
// PN-Counter row's replica columns.
// `--events`: one repetition per shape with JANUS_TRACE_ADOPT set, so the library reports its launches by hipEvents.
// usage: bench_adopt [--events] [--shape 1|2]
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "janus_gpu.h"

namespace {

using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count() * 1e3; }

void check(int rc, const char* what) {
    if (rc == JG_OK) return;
    char buf[512];
    jg_last_error(buf, sizeof buf);
    std::fprintf(stderr, "%s failed: [%d] %s\n", what, rc, buf);
    std::exit(1);
}
void require(bool ok, const char* what) {
    if (ok) return;
    std::fprintf(stderr, "mismatch: %s\n", what);
    std::exit(2);
}
double median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

struct GuidHash {
    size_t operator()(const jg_guid& g) const {
        uint64_t x = g.lo ^ (g.hi * 0x9E3779B97F4A7C15ull);
        x ^= x >> 31, x *= 0xBF58476D1CE4E5B9ull, x ^= x >> 29;
        return (size_t)x;
    }
};
struct GuidEq {
    bool operator()(const jg_guid& a, const jg_guid& b) const { return a.lo == b.lo && a.hi == b.hi; }
};

const jg_guid kStableRep{0x57AB1E, 1}, kProspRep{0x940590, 2};

struct Shape {  // what node 0 ships
    uint64_t K;
    std::vector<jg_guid> uid;
    std::vector<uint8_t> type;
    std::vector<uint64_t> koff{0};
    std::string kbytes, state;
};

struct Joiner {  // an empty node: key space, stable and prospective copies
    jg_keyspace* ks = nullptr;
    jg_pnc *sp = nullptr, *pp = nullptr;
    jg_orset *so = nullptr, *po = nullptr;
    jg_node *stable = nullptr, *prosp = nullptr;
    std::vector<uint32_t> idx;  // per journal record, as the run assigned it
    double t_receive = 0, t_prosp = 0, t_stable = 0;
    Joiner(jg_ctx* ctx, const Shape& s) {
        check(jg_keyspace_create(ctx, s.K + 16, s.kbytes.size() + s.K * 40 + 4096, &ks), "jg_keyspace_create");
        check(jg_pnc_create(ctx, s.K / 2 + 1, 2, 8, &sp), "jg_pnc_create");
        check(jg_pnc_create(ctx, s.K / 2 + 1, 2, 8, &pp), "jg_pnc_create");
        check(jg_orset_create(ctx, 0, 0, &so), "jg_orset_create");
        check(jg_orset_create(ctx, 0, 0, &po), "jg_orset_create");
        check(jg_node_create(sp, so, &stable), "jg_node_create");
        check(jg_node_create(pp, po, &prosp), "jg_node_create");
    }
    ~Joiner() {
        jg_node_destroy(stable), jg_node_destroy(prosp), jg_orset_destroy(so), jg_orset_destroy(po), jg_pnc_destroy(sp), jg_pnc_destroy(pp);
        jg_keyspace_destroy(ks);
    }
    Joiner(const Joiner&) = delete;
    void receive(const Shape& s) {
        const auto t0 = Clock::now();
        const uint64_t off[2] = {0, s.state.size()};
        uint64_t n_new = 0;
        check(jg_keyspace_receive(ks, 1, off, reinterpret_cast<const uint8_t*>(s.state.data()), 0, nullptr, nullptr, &n_new), "jg_keyspace_receive");
        require(n_new == s.K, "every key is learnt");
        t_receive = ms_since(t0);
    }
    double total() const { return t_receive + t_prosp + t_stable; }
};

void device_way(Joiner& j, const Shape& s) {
    j.receive(s);
    auto t0 = Clock::now();
    {
        std::vector<jg_guid> rep(s.K, kProspRep);
        std::vector<uint8_t> status(s.K);
        check(jg_node_create_uids(j.prosp, s.K, s.uid.data(), s.type.data(), rep.data(), 0, status.data(), nullptr), "jg_node_create_uids");
    }
    j.t_prosp = ms_since(t0);
    t0 = Clock::now();
    {
        std::vector<jg_guid> rep(s.K, kStableRep);
        std::vector<uint8_t> status(s.K);
        j.idx.resize(s.K);
        check(jg_node_adopt_keys(j.stable, j.prosp, j.ks, 0, s.K, rep.data(), 0, status.data(), nullptr, j.idx.data()), "jg_node_adopt_keys");
        require(std::count(status.begin(), status.end(), (uint8_t)JG_A_ADOPTED) == (long)s.K, "every record is adopted");
    }
    j.t_stable = ms_since(t0);
}

// jg_node_register + jg_pnc_intern at the rows a host allocator hands out, in order
void register_at(jg_node* node, jg_pnc* pnc, uint64_t n, const jg_guid* uid, const uint8_t* type, const jg_guid& replica, std::vector<uint32_t>& idx) {
    uint32_t next[2] = {0, 0};
    idx.resize(n);
    std::vector<uint32_t> rows;
    for (uint64_t i = 0; i < n; ++i) {
        idx[i] = next[type[i]]++;
        if (type[i] == 0) rows.push_back(idx[i]);
    }
    check(jg_node_register(node, n, uid, type, idx.data()), "jg_node_register");
    std::vector<jg_guid> rep(rows.size(), replica);
    std::vector<uint32_t> col(rows.size());
    check(jg_pnc_intern(pnc, rows.size(), rows.data(), rep.data(), col.data()), "jg_pnc_intern");
}

void parent_way(Joiner& j, const Shape& s) {
    j.receive(s);
    auto t0 = Clock::now();
    std::unordered_map<jg_guid, uint8_t, GuidHash, GuidEq> types;  // ReplicationManager's uid -> type, kept by the caller
    {
        types.reserve(s.K);
        for (uint64_t i = 0; i < s.K; ++i) types.emplace(s.uid[i], s.type[i]);
        std::vector<uint32_t> idx;
        register_at(j.prosp, j.pp, s.K, s.uid.data(), s.type.data(), kProspRep, idx);
    }
    j.t_prosp = ms_since(t0);
    t0 = Clock::now();
    {
        uint64_t to = 0, nb = 0;
        check(jg_keyspace_new_keys(j.ks, 0, &to, &nb, nullptr, nullptr, nullptr, nullptr), "jg_keyspace_new_keys (size)");
        std::vector<uint64_t> off(to + 1);
        std::vector<uint8_t> bytes(nb + 1), status(to), type(to);
        std::vector<jg_guid> guid(to);
        check(jg_keyspace_new_keys(j.ks, 0, &to, &nb, off.data(), bytes.data(), guid.data(), status.data()), "jg_keyspace_new_keys");
        for (uint64_t r = 0; r < to; ++r) type[r] = types.at(guid[r]);  // GetCRDTType
        register_at(j.stable, j.sp, to, guid.data(), type.data(), kStableRep, j.idx);
    }
    j.t_stable = ms_since(t0);
}

// both ways left the same nodes behind
void compare(const Shape& s, Joiner& a, Joiner& b, const char* what) {
    require(a.idx == b.idx, what);
    for (int copy = 0; copy < 2; ++copy) {
        uint32_t ar = 0, as = 0, br = 0, bs = 0;
        check(jg_node_next_idx(copy ? a.prosp : a.stable, &ar, &as), "jg_node_next_idx");
        check(jg_node_next_idx(copy ? b.prosp : b.stable, &br, &bs), "jg_node_next_idx");
        require(ar == br && as == bs && ar + as == s.K, what);
        std::vector<int64_t> va(s.K), vb(s.K);
        std::vector<uint8_t> sa(s.K), sb(s.K), ka(s.K), kb(s.K);
        check(jg_node_query_keys(copy ? a.prosp : a.stable, a.ks, s.K, s.koff.data(), reinterpret_cast<const uint8_t*>(s.kbytes.data()), nullptr, nullptr, nullptr,
                                 va.data(), sa.data(), ka.data(), nullptr), "jg_node_query_keys");
        check(jg_node_query_keys(copy ? b.prosp : b.stable, b.ks, s.K, s.koff.data(), reinterpret_cast<const uint8_t*>(s.kbytes.data()), nullptr, nullptr, nullptr,
                                 vb.data(), sb.data(), kb.data(), nullptr), "jg_node_query_keys");
        require(sa == sb && ka == kb && va == vb && ka == s.type, what);
        std::vector<uint32_t> rows(ar), na(ar), nb(ar);
        for (uint32_t r = 0; r < ar; ++r) rows[r] = r;
        std::vector<jg_guid> ca(2ull * ar), cb(2ull * ar);
        check(jg_pnc_columns(copy ? a.pp : a.sp, ar, rows.data(), ca.data(), na.data()), "jg_pnc_columns");
        check(jg_pnc_columns(copy ? b.pp : b.sp, ar, rows.data(), cb.data(), nb.data()), "jg_pnc_columns");
        require(na == nb && !std::memcmp(ca.data(), cb.data(), ca.size() * sizeof(jg_guid)) && (ar == 0 || na[0] == 1), what);
    }
}

void run(jg_ctx* ctx, const char* what, const Shape& s, bool events, int reps) {
    const int warm = 1;
    if (events) reps = 1;
    std::vector<double> t, b1, b2, tr, tp, ts, br, bp, bs;
    for (int r = 0; r < warm + reps; ++r) {
        Joiner x(ctx, s), y(ctx, s), z(ctx, s);
        parent_way(x, s);
        device_way(y, s);
        parent_way(z, s);
        compare(s, y, x, what);
        compare(s, y, z, what);
        if (r < warm) continue;
        t.push_back(y.total()), b1.push_back(x.total()), b2.push_back(z.total());
        tr.push_back(y.t_receive), tp.push_back(y.t_prosp), ts.push_back(y.t_stable);
        br.push_back(x.t_receive), bp.push_back(x.t_prosp), bs.push_back(x.t_stable);
    }
    const double m = median(t), m1 = median(b1), m2 = median(b2), base = std::min(m1, m2), spread = std::abs(m1 - m2);
    std::printf("%s: device way %.3f ms; parent's way %.3f / %.3f ms (A/A spread %.3f ms = %.1f%%); device way is %.2fx the parent's way: %s\n", what, m, m1,
                m2, spread, 100 * spread / base, m / base, m <= base + spread ? "within the bar" : "SLOWER than the parent's way");
    std::printf("    device way: receive %.3f ms, create_uids (prospective) %.3f ms, adopt_keys (stable) %.3f ms\n", median(tr), median(tp), median(ts));
    std::printf("    parent's way: receive %.3f ms, map + register + intern (prospective) %.3f ms, new_keys + map + register + intern (stable) %.3f ms\n",
                median(br), median(bp), median(bs));
}

Shape make_shape(jg_ctx* ctx, uint64_t K) {
    Shape s;
    s.K = K;
    s.uid.resize(K), s.type.resize(K);
    for (uint64_t i = 0; i < K; ++i) {
        s.kbytes += "key-" + std::to_string(i), s.koff.push_back(s.kbytes.size());
        s.uid[i] = jg_guid{0x1000000 + i, 0xC0FFEE0000000000ull ^ (i * 0x9E3779B97F4A7C15ull)};
        s.type[i] = (uint8_t)(i & 1);
    }
    jg_keyspace* ks = nullptr;
    check(jg_keyspace_create(ctx, K + 16, s.kbytes.size() + K * 40 + 4096, &ks), "jg_keyspace_create");
    check(jg_keyspace_create_keys(ks, K, s.koff.data(), reinterpret_cast<const uint8_t*>(s.kbytes.data()), s.uid.data(), nullptr), "jg_keyspace_create_keys");
    jg_tpset* set = nullptr;
    check(jg_keyspace_set(ks, &set), "jg_keyspace_set");
    uint64_t nb = 0;
    check(jg_tpset_encode_json(set, &nb, nullptr, 0), "jg_tpset_encode_json (size)");
    s.state.resize(nb);
    check(jg_tpset_encode_json(set, &nb, reinterpret_cast<uint8_t*>(s.state.data()), nb), "jg_tpset_encode_json");
    jg_keyspace_destroy(ks);
    return s;
}

}  // namespace

int main(int argc, char** argv) {
    bool events = false;
    int only = 0;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--events")) events = true;
        else if (!std::strcmp(argv[i], "--shape") && i + 1 < argc) only = std::atoi(argv[++i]);
    }
    if (events) setenv("JANUS_TRACE_ADOPT", "1", 1);  // the library latches it at its first call
    jg_ctx* ctx = nullptr;
    check(jg_open(0, &ctx), "jg_open");
    if (!only || only == 1) run(ctx, "(1) 1,000,000 learnt keys, half PN-Counter, half OR-Set", make_shape(ctx, 1000000), events, 5);
    if (!only || only == 2) run(ctx, "(2) 10,000 learnt keys, half PN-Counter, half OR-Set", make_shape(ctx, 10000), events, 9);
    jg_close(ctx);
    return 0;
}
