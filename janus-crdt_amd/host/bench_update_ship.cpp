// host/bench_update_ship.cpp — client writes by key name that ship every snapshot in one call (jg_node_update_keys_ship,
// csrc/update.hip) beside the parent's way: jg_keyspace_lookup -> one thread of unordered_map<guid, (type,
// idx)> -> the rounds on the host (a Clear after a shipping command of its set starts one) -> per round
// jg_orset_apply_ops_names + jg_orset_encode_json at the limits, and jg_pnc_apply_ops_encode for the PN-Counter half.
//   (1) ORSetWorkload writes: 10,000 sets filled as in bench_names, a 200k-command batch of Adds of random 5-character
//       names, a set cleared when it holds 50 (ORSetWorkload.cs:37-50)
//   (2) mixed: half C1 "i" commands (100 PN-Counter keys x 4 int32 columns, 4 interned replicas), half shape (1)
// each with snap all 1 (every command ships) and all 2 (the latest state per object; the parent's PN-Counter call has no
// such rule and encodes every command, its OR-Set side ships the last command of each set).
// bench_update's method: each way has stores of its own over one key space (one by key, two for the two runs of the
// parent's way); every repetition applies the same batch to all three, and the bytes, hashes and OR-Set stores are compared
// afterwards, outside the timed part.  Wall time of the calls a caller makes; 2 warm-ups, median of 7, the ways alternating;
// the distance of the parent's two medians is the A/A spread a difference has to exceed.  The parent's way is not charged
// for merging its two kinds' messages back into command order.
// `--events`: one repetition per shape with JANUS_TRACE_UPDATE set: the library reports its steps on stderr.
// usage: bench_update_ship [--events] [--shape 1|2] [--snap 1|2]
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
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

const char kChars[] = "abcdefghijklmnorqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789";  // sic (BenchmarkWorload.cs:151)

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
struct Ref { uint8_t type; uint32_t idx; };
using UidMap = std::unordered_map<jg_guid, Ref, GuidHash, GuidEq>;  // the caller's Dictionary<Guid, ...>

struct Strings {
    std::vector<uint64_t> off{0};
    std::string bytes;
    void push(const std::string& s) { bytes += s, off.push_back(bytes.size()); }
    uint64_t n() const { return off.size() - 1; }
    const uint8_t* data() const { return reinterpret_cast<const uint8_t*>(bytes.empty() ? "" : bytes.data()); }
};

struct Copy {
    jg_pnc* pnc = nullptr;
    jg_orset* ors = nullptr;
    jg_node* node = nullptr;
};
struct World {
    jg_ctx* ctx;
    jg_keyspace* ks = nullptr;
    Copy c[3];  // 0: by key, 1 and 2: the parent's way
    UidMap uids;
    void make(uint64_t pnc_keys) {
        for (Copy& x : c) {
            if (pnc_keys) check(jg_pnc_create(ctx, pnc_keys, 4, 4, &x.pnc), "jg_pnc_create");
            check(jg_orset_create(ctx, 0, 0, &x.ors), "jg_orset_create");
            check(jg_node_create(x.pnc, x.ors, &x.node), "jg_node_create");
        }
    }
    void destroy() {
        for (Copy& x : c) {
            jg_node_destroy(x.node);
            if (x.pnc) jg_pnc_destroy(x.pnc);
            jg_orset_destroy(x.ors);
        }
        jg_keyspace_destroy(ks);
    }
    void add_keys(const char* prefix, uint64_t n, uint8_t type) {
        Strings k;
        std::vector<jg_guid> g(n);
        std::vector<uint8_t> t(n, type);
        std::vector<uint32_t> idx(n);
        for (uint64_t i = 0; i < n; ++i) {
            k.push(prefix + std::to_string(i));
            g[i] = jg_guid{0x1000000 + i * 2 + type, 0xC0FFEE0000000000ull ^ (i * 0x9E3779B97F4A7C15ull)};
            idx[i] = (uint32_t)i;
            uids.emplace(g[i], Ref{type, idx[i]});
        }
        check(jg_keyspace_create_keys(ks, n, k.off.data(), k.data(), g.data(), nullptr), "jg_keyspace_create_keys");
        for (Copy& x : c) check(jg_node_register(x.node, n, g.data(), t.data(), idx.data()), "jg_node_register");
        if (type == 0) {  // 4 interned replicas per row
            std::vector<uint32_t> rows(n * 4), col(n * 4);
            std::vector<jg_guid> rep(n * 4);
            for (uint64_t i = 0; i < n * 4; ++i) rows[i] = (uint32_t)(i / 4), rep[i] = jg_guid{0xABCD0000 + i % 4, 0x1234567800000000ull + i % 4};
            for (Copy& x : c) check(jg_pnc_intern(x.pnc, rows.size(), rows.data(), rep.data(), col.data()), "jg_pnc_intern");
        }
    }
};

struct Batch {  // "i" commands (flag 3) and OR-Set Adds (flag 1) / Clears (op 3, flag 0), in one order
    Strings keys, elems;
    std::vector<uint8_t> op, flag;
    std::vector<int64_t> amount;
    std::vector<uint64_t> lo, hi;
};
struct Shipped {  // per command: where its bytes are in the way's arena (an empty range: none) and its hash
    std::vector<uint8_t> arena;  // kept from one repetition to the next, as a caller keeps its buffers: grown in the warm-ups
    std::vector<uint64_t> pos, len;
    std::vector<uint8_t> sha;
    uint64_t bytes = 0;
    uint32_t rounds = 0;
    void reset(uint64_t n) { pos.assign(n, 0), len.assign(n, 0), sha.assign(n * 32, 0), bytes = 0, rounds = 0; }
    uint8_t* room(uint64_t more) {  // `more` bytes behind the `bytes` in use
        if (arena.size() < bytes + more) arena.resize((bytes + more) + (bytes + more) / 4);
        return arena.data() + bytes;
    }
    const uint8_t* at(uint64_t i) const { return arena.data() + pos[i]; }
};

double parent_way(World& w, Copy& c, const Batch& b, uint8_t snap_all, Shipped& s) {
    const uint64_t n = b.keys.n();
    s.reset(n);
    const auto t0 = Clock::now();
    std::vector<jg_guid> guid(n);
    std::vector<uint8_t> found(n);
    check(jg_keyspace_lookup(w.ks, n, b.keys.off.data(), b.keys.data(), guid.data(), found.data()), "jg_keyspace_lookup");
    std::vector<Ref> ref(n);
    for (uint64_t i = 0; i < n; ++i) {
        const auto it = found[i] ? w.uids.find(guid[i]) : w.uids.end();
        require(it != w.uids.end(), "every benchmark key resolves");
        ref[i] = it->second;
    }
    // who ships among the OR-Set commands, and the rounds
    std::vector<uint32_t> oi, pi;
    for (uint64_t i = 0; i < n; ++i) (ref[i].type ? oi : pi).push_back((uint32_t)i);
    std::unordered_map<uint32_t, uint32_t> last;  // snap 2: a set's last command
    if (snap_all == 2)
        for (uint32_t i : oi) last[ref[i].idx] = i;
    struct PerSet { uint32_t round = 0; bool open = false; };
    std::unordered_map<uint32_t, PerSet> per;
    std::vector<uint32_t> round(n, 0);
    std::vector<uint8_t> ships(n, 0);
    uint32_t rounds = oi.empty() ? 0 : 1;
    for (uint32_t i : oi) {
        PerSet& ps = per[ref[i].idx];
        if (b.op[i] == 3 && ps.open) ++ps.round, ps.open = false;
        round[i] = ps.round;
        rounds = std::max(rounds, ps.round + 1);
        ships[i] = snap_all == 1 || last[ref[i].idx] == i;
        if (ships[i]) ps.open = true;
    }
    s.rounds = rounds;
    for (uint32_t r = 0; r < rounds; ++r) {
        std::vector<uint32_t> cmd, set;
        std::vector<uint8_t> op, is_null;
        std::vector<uint64_t> lo, hi;
        Strings names;
        for (uint32_t i : oi) {
            if (round[i] != r) continue;
            cmd.push_back(i), set.push_back(ref[i].idx), op.push_back(b.op[i]), is_null.push_back(0), lo.push_back(b.lo[i]), hi.push_back(b.hi[i]);
            names.push(b.op[i] == 3 ? std::string() : b.elems.bytes.substr(b.elems.off[i], b.elems.off[i + 1] - b.elems.off[i]));
        }
        const uint64_t m = cmd.size();
        std::vector<uint8_t> res(m);
        std::vector<uint64_t> al(m), rl(m);
        check(jg_orset_apply_ops_names(c.ors, m, set.data(), op.data(), names.off.data(), names.data(), is_null.data(), lo.data(), hi.data(), res.data(),
                                       nullptr, al.data(), rl.data()), "jg_orset_apply_ops_names");
        std::vector<uint32_t> scmd, sset;
        std::vector<uint64_t> sal, srl;
        for (uint64_t k = 0; k < m; ++k)
            if (ships[cmd[k]]) scmd.push_back(cmd[k]), sset.push_back(set[k]), sal.push_back(al[k]), srl.push_back(rl[k]);
        const uint64_t q = scmd.size();
        if (!q) continue;
        std::vector<uint64_t> off(q + 1);
        check(jg_orset_encode_json(c.ors, q, sset.data(), sal.data(), srl.data(), off.data(), nullptr, 0, nullptr), "jg_orset_encode_json (size)");
        std::vector<uint8_t> sha(q * 32);
        check(jg_orset_encode_json(c.ors, q, sset.data(), sal.data(), srl.data(), off.data(), s.room(off[q] + 16), off[q] + 16, sha.data()),
              "jg_orset_encode_json");
        for (uint64_t k = 0; k < q; ++k) {
            s.pos[scmd[k]] = s.bytes + off[k], s.len[scmd[k]] = off[k + 1] - off[k];
            std::memcpy(s.sha.data() + 32 * scmd[k], sha.data() + 32 * k, 32);
        }
        s.bytes += off[q];
    }
    if (!pi.empty()) {
        const uint64_t m = pi.size();
        std::vector<uint32_t> row(m);
        std::vector<int64_t> amt(m);
        for (uint64_t k = 0; k < m; ++k) row[k] = ref[pi[k]].idx, amt[k] = b.amount[pi[k]];
        const std::vector<uint8_t> is_n(m, 0);
        std::vector<uint64_t> off(m + 1);
        std::vector<uint8_t> sha(m * 32);
        check(jg_pnc_apply_ops_encode(c.pnc, m, row.data(), 0, amt.data(), is_n.data(), off.data(), s.room(m * 512), m * 512, sha.data()),
              "jg_pnc_apply_ops_encode");
        for (uint64_t k = 0; k < m; ++k) {
            s.pos[pi[k]] = s.bytes + off[k], s.len[pi[k]] = off[k + 1] - off[k];
            std::memcpy(s.sha.data() + 32 * pi[k], sha.data() + 32 * k, 32);
        }
        s.bytes += off[m];
    }
    return ms_since(t0);
}

double by_key(World& w, Copy& c, const Batch& b, uint8_t snap_all, Shipped& s) {
    const uint64_t n = b.keys.n();
    s.reset(n);
    s.room(16);
    const auto t0 = Clock::now();
    const std::vector<uint8_t> snap(n, snap_all);
    std::vector<uint8_t> status(n), result(n);
    std::vector<uint64_t> off(n + 1);
    uint64_t nb = 0;
    check(jg_node_update_keys_ship(c.node, w.ks, n, b.keys.off.data(), b.keys.data(), b.op.data(), b.flag.data(), b.amount.data(), b.elems.off.data(),
                                   b.elems.data(), b.lo.data(), b.hi.data(), 0, snap.data(), status.data(), result.data(), nullptr, nullptr, nullptr, nullptr,
                                   off.data(), &nb, s.arena.data(), s.arena.size(), s.sha.data(), &s.rounds), "jg_node_update_keys_ship");
    if (nb > s.arena.size()) {  // (the warm-ups: the caller keeps the larger buffer)
        s.room(nb);
        check(jg_node_shipped(c.node, &nb, s.arena.data(), s.arena.size()), "jg_node_shipped");
    }
    const double ms = ms_since(t0);
    require(std::count(status.begin(), status.end(), JG_U_OK) == (long)n, "every command applies");
    for (uint64_t i = 0; i < n; ++i) s.pos[i] = off[i], s.len[i] = off[i + 1] - off[i];
    s.bytes = nb;
    return ms;
}

void compare(World& w, const Batch& b, uint8_t snap_all, const Shipped& k, const Shipped& p1, const Shipped& p2) {
    const uint64_t n = b.keys.n();
    require(k.rounds == p1.rounds && k.rounds == p2.rounds, "the rounds the library ran are the rounds of the rule");
    std::unordered_map<std::string, uint64_t> last;
    for (uint64_t i = 0; i < n; ++i) last[b.keys.bytes.substr(b.keys.off[i], b.keys.off[i + 1] - b.keys.off[i])] = i;
    for (uint64_t i = 0; i < n; ++i) {
        require(p1.len[i] == p2.len[i] && !std::memcmp(p1.at(i), p2.at(i), p1.len[i]), "the parent's two runs ship the same");
        const bool pnc = b.flag[i] == 3;
        if (snap_all == 2 && pnc) {  // the parent's PN-Counter call encodes every command; by key the row's last one ships, with those bytes
            const bool is_last = last[b.keys.bytes.substr(b.keys.off[i], b.keys.off[i + 1] - b.keys.off[i])] == i;
            require((k.len[i] != 0) == is_last, "a PN-Counter survivor is its row's last command");
            if (!is_last) continue;
        }
        require(k.len[i] == p1.len[i] && !std::memcmp(k.at(i), p1.at(i), k.len[i]) && !std::memcmp(k.sha.data() + 32 * i, p1.sha.data() + 32 * i, 32),
                "by key ships what the parent's way ships");
    }
    std::vector<jg_tagrec> a[3], r[3];
    for (int c = 0; c < 3; ++c) {
        uint64_t na = 0, nr = 0;
        check(jg_orset_size(w.c[c].ors, &na, &nr), "jg_orset_size");
        a[c].resize(na), r[c].resize(nr);
        check(jg_orset_read(w.c[c].ors, a[c].data(), na, r[c].data(), nr), "jg_orset_read");
    }
    const auto same = [](const std::vector<jg_tagrec>& x, const std::vector<jg_tagrec>& y) {
        return x.size() == y.size() && (x.empty() || !std::memcmp(x.data(), y.data(), x.size() * sizeof(jg_tagrec)));
    };
    require(same(a[0], a[1]) && same(a[0], a[2]) && same(r[0], r[1]) && same(r[0], r[2]), "the OR-Set stores agree");
    if (w.c[0].pnc) {
        std::vector<int64_t> v[3];
        std::vector<uint8_t> o[3];
        for (int c = 0; c < 3; ++c) {
            v[c].resize(100), o[c].resize(100);
            check(jg_pnc_values(w.c[c].pnc, nullptr, 100, v[c].data(), o[c].data()), "jg_pnc_values");
        }
        require(v[0] == v[1] && v[0] == v[2], "the PN-Counter stores agree");
    }
}

template <class Next> void run(const char* what, World& w, Next&& next, uint8_t snap_all, bool events) {
    const int warm = events ? 1 : 2, reps = events ? 1 : 7;
    std::vector<double> t, b1, b2;
    std::vector<Batch> batches;
    for (int r = 0; r < warm + reps; ++r) batches.push_back(next());
    Shipped k, p1, p2;
    uint64_t n = 0;
    for (int r = 0; r < warm + reps; ++r) {
        const Batch& b = batches[r];
        n = b.keys.n();
        const double x = parent_way(w, w.c[1], b, snap_all, p1);
        const double y = by_key(w, w.c[0], b, snap_all, k);
        const double z = parent_way(w, w.c[2], b, snap_all, p2);
        compare(w, b, snap_all, k, p1, p2);
        if (r >= warm) t.push_back(y), b1.push_back(x), b2.push_back(z);
    }
    const double m = median(t), m1 = median(b1), m2 = median(b2), base = std::min(m1, m2), spread = std::abs(m1 - m2);
    std::printf("%s, snap all %d: by key %.3f ms; parent's way %.3f / %.3f ms (A/A spread %.3f ms = %.1f%%); by key is %.2fx the parent's way: %s\n", what,
                snap_all, m, m1, m2, spread, 100 * spread / base, m / base, m <= base + spread ? "within the bar" : "SLOWER than the parent's way");
    std::printf("    %llu commands, %u rounds, %llu snapshot bytes by key = %.3f ms on the host link at 57 GB/s\n", (unsigned long long)n, k.rounds,
                (unsigned long long)k.bytes, k.bytes / 57e9 * 1e3);
    std::fflush(stdout);
}

}  // namespace

int main(int argc, char** argv) {
    bool events = false;
    int only = 0, only_snap = 0;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--events")) events = true;
        else if (!std::strcmp(argv[i], "--shape") && i + 1 < argc) only = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--snap") && i + 1 < argc) only_snap = std::atoi(argv[++i]);
    }
    if (events) setenv("JANUS_TRACE_UPDATE", "1", 1);  // the library latches it at its first call
    const uint64_t sets = 10000, batch = 200000, fill_batches = 15;  // bench_names' resident store
    std::mt19937_64 rng(2027);
    jg_ctx* ctx = nullptr;
    check(jg_open(0, &ctx), "jg_open");
    for (int shape = 1; shape <= 2; ++shape) {
        if (only && only != shape) continue;
        World w{ctx};
        check(jg_keyspace_create(ctx, sets + 256, sets * 64 + (1 << 14), &w.ks), "jg_keyspace_create");
        w.make(shape == 2 ? 100 : 0);
        w.add_keys("set", sets, 1);
        if (shape == 2) w.add_keys("key-", 100, 0);
        std::vector<uint32_t> live(sets, 0);  // names each set holds (Add of a random 5-character string, Clear at 50)
        const auto orset_command = [&](uint64_t& k, uint8_t& op, std::string& e) {
            k = rng() % sets;
            const bool clear = live[k] >= 50;  // ORSetWorkload.cs:37-50
            e.clear();
            if (clear) live[k] = 0;
            else {
                for (int c = 0; c < 5; ++c) e.push_back(kChars[rng() % (sizeof kChars - 1)]);
                ++live[k];
            }
            op = clear ? 3 : 1;
        };
        for (uint64_t f = 0; f < fill_batches; ++f) {
            std::vector<uint32_t> set;
            std::vector<uint8_t> op, is_null(batch, 0), res(batch);
            std::vector<uint64_t> lo, hi;
            Strings names;
            for (uint64_t i = 0; i < batch; ++i) {
                uint64_t k;
                uint8_t o;
                std::string e;
                orset_command(k, o, e);
                set.push_back((uint32_t)k), op.push_back(o), names.push(e), lo.push_back(rng() | 1), hi.push_back(rng());
            }
            for (Copy& c : w.c)
                check(jg_orset_apply_ops_names(c.ors, batch, set.data(), op.data(), names.off.data(), names.data(), is_null.data(), lo.data(), hi.data(),
                                               res.data(), nullptr, nullptr, nullptr), "jg_orset_apply_ops_names");
        }
        for (uint8_t snap = 1; snap <= 2; ++snap) {
            if (only_snap && only_snap != snap) continue;
            run(shape == 1 ? "(1) ORSetWorkload writes: 10,000 sets, 200k Adds and Clears by (key, element)"
                           : "(2) mixed: 100k C1 increments and 100k ORSetWorkload writes", w, [&] {
                Batch b;
                const uint64_t start = rng() % 100;
                for (uint64_t i = 0; i < batch; ++i) {
                    if (shape == 2 && i % 2 == 0) {
                        b.keys.push("key-" + std::to_string((start + i / 2) % 100)), b.elems.push(""), b.op.push_back(1), b.flag.push_back(3);
                        b.amount.push_back(1 + (int64_t)(rng() % 1000)), b.lo.push_back(0), b.hi.push_back(0);
                        continue;
                    }
                    uint64_t k;
                    uint8_t o;
                    std::string e;
                    orset_command(k, o, e);
                    b.keys.push("set" + std::to_string(k)), b.elems.push(e), b.op.push_back(o), b.flag.push_back(o == 3 ? 0 : 1);
                    b.amount.push_back(0), b.lo.push_back(rng() | 1), b.hi.push_back(rng());
                }
                return b;
            }, snap, events);
        }
        w.destroy();
    }
    jg_close(ctx);
    return 0;
}
