// host/bench_update_encode.cpp — client writes by key name that ship their PN-Counter snapshots in one call
// (jg_node_update_keys_encode, csrc/update.hip + csrc/pnc_encode.hip) beside the parent's way:
// jg_keyspace_lookup -> one thread of unordered_map<guid, row> -> jg_pnc_apply_ops_encode.
//   (1) C1 writes: 100 PN-Counter keys with 4 int32 columns, keys round-robin from a random start
//   (2) scaled: 1M PN-Counter keys x 64 int64 columns, uniformly random writes
// each at 250k "i" commands per call (one producer chunk) on rows of 4 interned replicas, with snap all 1 (every command
// ships) and all 2 (the latest state per object ships; the parent's call has no such rule and encodes every command).
// bench_update's method: each way has stores of its own over one key space (one for the call by key, two for the two runs
// of the parent's way); every repetition applies the same batch to all three, and the bytes, offsets, hashes and stores are
// compared afterwards, outside the timed part.  Wall time of the calls a caller makes; 2 warm-ups, median of 7, the ways
// alternating; the distance of the parent's two medians is the A/A spread a difference has to exceed.
// `--events`: one repetition per shape with JANUS_TRACE_UPDATE set: the library reports its steps by hipEvents on stderr.
// usage: bench_update_encode [--events] [--shape 1|2] [--snap 1|2]
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
using UidMap = std::unordered_map<jg_guid, uint32_t, GuidHash, GuidEq>;  // the caller's Dictionary<Guid, row>

struct Strings {
    std::vector<uint64_t> off{0};
    std::string bytes;
    void push(const std::string& s) { bytes += s, off.push_back(bytes.size()); }
    uint64_t n() const { return off.size() - 1; }
    const uint8_t* data() const { return reinterpret_cast<const uint8_t*>(bytes.data()); }
};

struct Copy {
    jg_pnc* pnc = nullptr;
    jg_node* node = nullptr;
};
struct World {
    jg_ctx* ctx;
    jg_keyspace* ks = nullptr;
    Copy c[3];  // 0: by key, 1 and 2: the parent's way
    UidMap uids;
    // n keys "key-<i>" on row i with `replicas` interned replica Guids each, on every copy
    void make(uint64_t n, uint32_t R, uint32_t eb, uint32_t replicas) {
        Strings k;
        std::vector<jg_guid> g(n);
        std::vector<uint8_t> t(n, 0);
        std::vector<uint32_t> idx(n);
        for (uint64_t i = 0; i < n; ++i) {
            k.push("key-" + std::to_string(i));
            g[i] = jg_guid{0x1000000 + i * 2, 0xC0FFEE0000000000ull ^ (i * 0x9E3779B97F4A7C15ull)};
            idx[i] = (uint32_t)i;
            uids.emplace(g[i], idx[i]);
        }
        check(jg_keyspace_create_keys(ks, n, k.off.data(), k.data(), g.data(), nullptr), "jg_keyspace_create_keys");
        std::vector<uint32_t> rows(n * replicas), col(n * replicas);
        std::vector<jg_guid> rep(n * replicas);
        for (uint64_t i = 0; i < n * replicas; ++i) rows[i] = (uint32_t)(i / replicas), rep[i] = jg_guid{0xABCD0000 + i % replicas, 0x1234567800000000ull + i % replicas};
        for (Copy& x : c) {
            check(jg_pnc_create(ctx, n, R, eb, &x.pnc), "jg_pnc_create");
            check(jg_node_create(x.pnc, nullptr, &x.node), "jg_node_create");
            check(jg_node_register(x.node, n, g.data(), t.data(), idx.data()), "jg_node_register");
            check(jg_pnc_intern(x.pnc, rows.size(), rows.data(), rep.data(), col.data()), "jg_pnc_intern");
        }
    }
    void destroy() {
        for (Copy& x : c) jg_node_destroy(x.node), jg_pnc_destroy(x.pnc);
        jg_keyspace_destroy(ks);
    }
};

struct Batch {
    Strings keys;
    std::vector<int64_t> amount;
};
struct Shipped {  // what one way returned for a batch
    std::vector<uint64_t> off;
    std::vector<uint8_t> bytes, sha;
};

double parent_way(World& w, Copy& c, const Batch& b, Shipped& s) {
    const uint64_t n = b.keys.n();
    s.off.assign(n + 1, 0), s.sha.assign(n * 32, 0), s.bytes.resize(n * 512);
    const auto t0 = Clock::now();
    std::vector<jg_guid> guid(n);
    std::vector<uint8_t> found(n);
    check(jg_keyspace_lookup(w.ks, n, b.keys.off.data(), b.keys.data(), guid.data(), found.data()), "jg_keyspace_lookup");
    std::vector<uint32_t> row(n);
    for (uint64_t i = 0; i < n; ++i) {
        const auto it = found[i] ? w.uids.find(guid[i]) : w.uids.end();
        require(it != w.uids.end(), "every benchmark key resolves");
        row[i] = it->second;
    }
    const std::vector<uint8_t> is_n(n, 0);
    check(jg_pnc_apply_ops_encode(c.pnc, n, row.data(), 0, b.amount.data(), is_n.data(), s.off.data(), s.bytes.data(), s.bytes.size(), s.sha.data()),
          "jg_pnc_apply_ops_encode");
    return ms_since(t0);
}

double by_key(World& w, Copy& c, const Batch& b, uint8_t snap_all, Shipped& s) {
    const uint64_t n = b.keys.n();
    s.off.assign(n + 1, 0), s.sha.assign(n * 32, 0), s.bytes.resize(n * 512);
    const auto t0 = Clock::now();
    const std::vector<uint8_t> op(n, 1), flag(n, 3), snap(n, snap_all);
    std::vector<uint8_t> status(n), result(n);
    check(jg_node_update_keys_encode(c.node, w.ks, n, b.keys.off.data(), b.keys.data(), op.data(), flag.data(), b.amount.data(), nullptr, nullptr, nullptr,
                                     nullptr, 0, snap.data(), status.data(), result.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                     s.off.data(), s.bytes.data(), s.bytes.size(), s.sha.data()),
          "jg_node_update_keys_encode");
    const double ms = ms_since(t0);
    require(std::count(status.begin(), status.end(), JG_U_OK) == (long)n, "every command applies");
    return ms;
}

void compare(World& w, const Batch& b, uint8_t snap_all, const Shipped& k, const Shipped& p1, const Shipped& p2, uint64_t n_keys, uint32_t R, uint32_t eb) {
    const uint64_t n = b.keys.n();
    require(p1.off == p2.off && p1.sha == p2.sha && !std::memcmp(p1.bytes.data(), p2.bytes.data(), p1.off[n]), "the parent's two runs ship the same");
    if (snap_all == 1) {
        require(k.off == p1.off && k.sha == p1.sha && !std::memcmp(k.bytes.data(), p1.bytes.data(), k.off[n]), "by key ships what the parent's way ships");
    } else {  // the latest command of each row ships, with the bytes the parent's way wrote for that command
        std::unordered_map<std::string, uint64_t> last;
        for (uint64_t i = 0; i < n; ++i) last[b.keys.bytes.substr(b.keys.off[i], b.keys.off[i + 1] - b.keys.off[i])] = i;
        uint64_t shipped = 0;
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t len = k.off[i + 1] - k.off[i];
            if (!len) continue;
            ++shipped;
            require(last[b.keys.bytes.substr(b.keys.off[i], b.keys.off[i + 1] - b.keys.off[i])] == i, "a survivor is its row's last command");
            require(len == p1.off[i + 1] - p1.off[i] && !std::memcmp(k.bytes.data() + k.off[i], p1.bytes.data() + p1.off[i], len) &&
                        !std::memcmp(k.sha.data() + 32 * i, p1.sha.data() + 32 * i, 32), "a survivor's bytes and hash are the parent's for that command");
        }
        require(shipped == last.size(), "one survivor per row");
    }
    std::vector<uint32_t> rows;  // the rows of the batch's first 4096 commands
    for (uint64_t i = 0; i < std::min<uint64_t>(n, 4096); ++i) rows.push_back((uint32_t)std::stoul(b.keys.bytes.substr(b.keys.off[i] + 4, b.keys.off[i + 1] - b.keys.off[i] - 4)));
    std::vector<uint8_t> P[3], N[3], o[3];
    std::vector<int64_t> v[3];
    for (int c = 0; c < 3; ++c) {
        P[c].resize(rows.size() * R * eb), N[c].resize(rows.size() * R * eb), v[c].resize(n_keys), o[c].resize(n_keys);
        check(jg_pnc_read_rows(w.c[c].pnc, rows.data(), rows.size(), P[c].data(), N[c].data()), "jg_pnc_read_rows");
        check(jg_pnc_values(w.c[c].pnc, nullptr, n_keys, v[c].data(), o[c].data()), "jg_pnc_values");
    }
    require(P[0] == P[1] && P[0] == P[2] && N[0] == N[1] && N[0] == N[2] && v[0] == v[1] && v[0] == v[2] && o[0] == o[1] && o[0] == o[2], "the stores agree");
}

template <class Next> void run(const char* what, World& w, Next&& next, uint8_t snap_all, uint64_t n_keys, uint32_t R, uint32_t eb, bool events) {
    const int warm = events ? 1 : 2, reps = events ? 1 : 7;
    std::vector<double> t, b1, b2;
    std::vector<Batch> batches;
    for (int r = 0; r < warm + reps; ++r) batches.push_back(next());
    Shipped k, p1, p2;
    uint64_t n = 0, bytes = 0;
    for (int r = 0; r < warm + reps; ++r) {
        const Batch& b = batches[r];
        n = b.keys.n();
        const double x = parent_way(w, w.c[1], b, p1);
        const double y = by_key(w, w.c[0], b, snap_all, k);
        const double z = parent_way(w, w.c[2], b, p2);
        bytes = k.off[n];
        compare(w, b, snap_all, k, p1, p2, n_keys, R, eb);
        if (r >= warm) t.push_back(y), b1.push_back(x), b2.push_back(z);
    }
    const double m = median(t), m1 = median(b1), m2 = median(b2), base = std::min(m1, m2), spread = std::abs(m1 - m2);
    std::printf("%s, snap all %d: by key %.3f ms; parent's way %.3f / %.3f ms (A/A spread %.3f ms = %.1f%%); by key is %.2fx the parent's way: %s\n", what,
                snap_all, m, m1, m2, spread, 100 * spread / base, m / base, m <= base + spread ? "within the bar" : "SLOWER than the parent's way");
    std::printf("    %llu commands, %llu snapshot bytes by key\n", (unsigned long long)n, (unsigned long long)bytes);
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
    const uint64_t nq = 250000;
    std::mt19937_64 rng(2026);
    jg_ctx* ctx = nullptr;
    check(jg_open(0, &ctx), "jg_open");
    for (int shape = 1; shape <= 2; ++shape) {
        if (only && only != shape) continue;
        const uint64_t K = shape == 1 ? 100 : 1000000;
        const uint32_t R = shape == 1 ? 4 : 64, eb = shape == 1 ? 4 : 8;
        World w{ctx};
        check(jg_keyspace_create(ctx, K + 28, K * 64 + (1 << 14), &w.ks), "jg_keyspace_create");
        w.make(K, R, eb, 4);
        for (uint8_t snap = 1; snap <= 2; ++snap) {
            if (only_snap && only_snap != snap) continue;
            run(shape == 1 ? "(1) C1 writes: 100 keys x 4 int32 columns, 250k increments" : "(2) scaled: 1M keys x 64 int64 columns, 250k random writes", w, [&] {
                Batch b;
                const uint64_t start = rng() % K;
                for (uint64_t i = 0; i < nq; ++i)
                    b.keys.push("key-" + std::to_string(shape == 1 ? (start + i) % K : rng() % K)), b.amount.push_back(1 + (int64_t)(rng() % 1000));
                return b;
            }, snap, K, R, eb, events);
        }
        w.destroy();
    }
    jg_close(ctx);
    return 0;
}
