// host/bench_update.cpp — client writes by key name in one call (jg_node_update_keys, csrc/update.hip)
// beside the parent's way: jg_keyspace_lookup -> one thread of unordered_map<guid, (type, idx)> -> jg_pnc_apply_ops /
// jg_orset_apply_ops_names.
//   (1) C1 writes: 100 PN-Counter keys with 4 int32 columns, 1M "i" commands per call, keys round-robin from a random start
//   (2) scaled: 1M PN-Counter keys x 64 int64 columns, 1M uniformly random writes
//   (3) ORSetWorkload writes: 10,000 sets filled as in bench_names, one batch of 200k Adds by (key, element)
// Writes change the store, so each way has stores of its own over one key space: one for the call by key, two for the two
// runs of the parent's way; every repetition applies the same batch to all three and the stores are compared afterwards
// (outside the timed part).  Wall time of the calls a caller makes; 2 warm-ups, median of 7, the ways alternating; the
// distance of the parent's two medians is the A/A spread a difference has to exceed.
// `--events`: one repetition per shape with JANUS_TRACE_UPDATE set, so the library reports the upload, the launches and
// the copies out by hipEvents on stderr.
// usage: bench_update [--events] [--shape 1|2|3]
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
    const uint8_t* data() const { return reinterpret_cast<const uint8_t*>(bytes.data()); }
};

struct Copy {  // one way's stores and node
    jg_pnc* pnc = nullptr;
    jg_orset* ors = nullptr;
    jg_node* node = nullptr;
};
struct World {
    jg_ctx* ctx;
    jg_keyspace* ks = nullptr;
    Copy c[3];  // 0: by key, 1 and 2: the parent's way
    UidMap uids;
    void make(uint64_t pnc_keys, uint32_t R, uint32_t eb, bool orset) {
        for (Copy& x : c) {
            if (pnc_keys) check(jg_pnc_create(ctx, pnc_keys, R, eb, &x.pnc), "jg_pnc_create");
            if (orset) check(jg_orset_create(ctx, 0, 0, &x.ors), "jg_orset_create");
            check(jg_node_create(x.pnc, x.ors, &x.node), "jg_node_create");
        }
    }
    void destroy() {
        for (Copy& x : c) {
            jg_node_destroy(x.node);
            if (x.pnc) jg_pnc_destroy(x.pnc);
            if (x.ors) jg_orset_destroy(x.ors);
        }
        jg_keyspace_destroy(ks);
    }
    // n keys named prefix + index, guid from the index, registered as `type` with idx = index on every copy
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
    }
};

struct Batch {  // one kind per batch: PN-Counter "i" commands (elems empty) or OR-Set Adds
    Strings keys, elems;
    std::vector<int64_t> amount;
    std::vector<uint64_t> lo, hi;
    bool orset = false;
};

// the parent's way: lookup, the caller's dictionary on one thread, the store's own entry point
double parent_way(World& w, Copy& c, const Batch& b) {
    const uint64_t n = b.keys.n();
    const auto t0 = Clock::now();
    std::vector<jg_guid> guid(n);
    std::vector<uint8_t> found(n);
    check(jg_keyspace_lookup(w.ks, n, b.keys.off.data(), b.keys.data(), guid.data(), found.data()), "jg_keyspace_lookup");
    std::vector<uint32_t> idx(n);
    for (uint64_t i = 0; i < n; ++i) {
        const auto it = found[i] ? w.uids.find(guid[i]) : w.uids.end();
        require(it != w.uids.end() && it->second.type == (b.orset ? 1 : 0), "every benchmark key resolves");
        idx[i] = it->second.idx;
    }
    if (!b.orset) {
        const std::vector<uint32_t> col(n, 0);
        const std::vector<uint8_t> is_n(n, 0);
        check(jg_pnc_apply_ops(c.pnc, n, idx.data(), col.data(), b.amount.data(), is_n.data()), "jg_pnc_apply_ops");
    } else {
        const std::vector<uint8_t> op(n, 1), is_null(n, 0);
        std::vector<uint8_t> res(n);
        check(jg_orset_apply_ops_names(c.ors, n, idx.data(), op.data(), b.elems.off.data(), b.elems.data(), is_null.data(), b.lo.data(), b.hi.data(),
                                       res.data(), nullptr, nullptr, nullptr), "jg_orset_apply_ops_names");
    }
    return ms_since(t0);
}

double by_key(World& w, Copy& c, const Batch& b) {
    const uint64_t n = b.keys.n();
    const auto t0 = Clock::now();
    const std::vector<uint8_t> op(n, 1), flag(n, b.orset ? 1 : 3);
    std::vector<uint8_t> status(n), result(n);
    check(jg_node_update_keys(c.node, w.ks, n, b.keys.off.data(), b.keys.data(), op.data(), flag.data(), b.orset ? nullptr : b.amount.data(),
                              b.orset ? b.elems.off.data() : nullptr, b.orset ? b.elems.data() : nullptr, b.orset ? b.lo.data() : nullptr,
                              b.orset ? b.hi.data() : nullptr, 0, status.data(), result.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr),
          "jg_node_update_keys");
    const double ms = ms_since(t0);
    require(std::count(status.begin(), status.end(), JG_U_OK) == (long)n, "every command applies");
    return ms;
}

// the stores of the three copies hold the same (PN-Counter: `rows` sampled rows cell by cell and every key's value)
void compare(World& w, const std::vector<uint32_t>& rows, uint64_t n_keys, uint32_t R, uint32_t eb, const char* what) {
    if (w.c[0].pnc) {
        std::vector<uint8_t> P[3], N[3];
        std::vector<int64_t> v[3];
        std::vector<uint8_t> o[3];
        for (int k = 0; k < 3; ++k) {
            P[k].resize(rows.size() * R * eb), N[k].resize(rows.size() * R * eb), v[k].resize(n_keys), o[k].resize(n_keys);
            check(jg_pnc_read_rows(w.c[k].pnc, rows.data(), rows.size(), P[k].data(), N[k].data()), "jg_pnc_read_rows");
            check(jg_pnc_values(w.c[k].pnc, nullptr, n_keys, v[k].data(), o[k].data()), "jg_pnc_values");
        }
        require(P[0] == P[1] && P[0] == P[2] && N[0] == N[1] && N[0] == N[2] && v[0] == v[1] && v[0] == v[2] && o[0] == o[1] && o[0] == o[2], what);
    }
    if (w.c[0].ors) {
        std::vector<jg_tagrec> a[3], r[3];
        for (int k = 0; k < 3; ++k) {
            uint64_t na = 0, nr = 0;
            check(jg_orset_size(w.c[k].ors, &na, &nr), "jg_orset_size");
            a[k].resize(na), r[k].resize(nr);
            check(jg_orset_read(w.c[k].ors, a[k].data(), na, r[k].data(), nr), "jg_orset_read");
        }
        const auto same = [](const std::vector<jg_tagrec>& x, const std::vector<jg_tagrec>& y) {
            return x.size() == y.size() && (x.empty() || !std::memcmp(x.data(), y.data(), x.size() * sizeof(jg_tagrec)));
        };
        require(same(a[0], a[1]) && same(a[0], a[2]) && same(r[0], r[1]) && same(r[0], r[2]), what);
    }
}

// `next`: the batch of the next repetition (the same for the three copies)
template <class Next> void run(const char* what, World& w, Next&& next, uint64_t n_keys, uint32_t R, uint32_t eb, bool events) {
    const int warm = events ? 1 : 2, reps = events ? 1 : 7;
    std::vector<double> t, b1, b2;
    uint64_t n = 0, up = 0;
    std::vector<Batch> batches;  // made before the timed loop: building one frees and faults a few hundred MB of host memory
    for (int r = 0; r < warm + reps; ++r) batches.push_back(next());
    for (int r = 0; r < warm + reps; ++r) {
        const Batch& b = batches[r];
        n = b.keys.n();
        up = b.keys.bytes.size() + (n + 1) * 8 + 2 * n + (b.orset ? b.elems.bytes.size() + (n + 1) * 8 + 16 * n : 8 * n);
        const double x = parent_way(w, w.c[1], b);
        const double y = by_key(w, w.c[0], b);
        const double z = parent_way(w, w.c[2], b);
        std::vector<uint32_t> rows;  // the rows of the batch's first 4096 commands
        if (!b.orset)
            for (uint64_t i = 0; i < std::min<uint64_t>(n, 4096); ++i) rows.push_back((uint32_t)std::stoul(b.keys.bytes.substr(b.keys.off[i] + 4, b.keys.off[i + 1] - b.keys.off[i] - 4)));
        compare(w, rows, n_keys, R, eb, what);
        if (r >= warm) t.push_back(y), b1.push_back(x), b2.push_back(z);
    }
    const double m = median(t), m1 = median(b1), m2 = median(b2), base = std::min(m1, m2), spread = std::abs(m1 - m2);
    std::printf("%s: by key %.3f ms; parent's way %.3f / %.3f ms (A/A spread %.3f ms = %.1f%%); by key is %.2fx the parent's way: %s\n", what, m, m1, m2,
                spread, 100 * spread / base, m / base, m <= std::max(m1, m2) + spread ? "within the bar" : "SLOWER than the parent's way");
    std::printf("    %llu commands; %llu bytes up + %llu bytes down = %.4f ms on the host link at 57 GB/s\n", (unsigned long long)n, (unsigned long long)up,
                (unsigned long long)(n * 6), (up + n * 6) / 57e9 * 1e3);
    std::fflush(stdout);
}

}  // namespace

int main(int argc, char** argv) {
    bool events = false;
    int only = 0;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--events")) events = true;
        else if (!std::strcmp(argv[i], "--shape") && i + 1 < argc) only = std::atoi(argv[++i]);
    }
    if (events) setenv("JANUS_TRACE_UPDATE", "1", 1);  // the library latches it at its first call
    const uint64_t nq = 1000000;
    std::mt19937_64 rng(2025);
    jg_ctx* ctx = nullptr;
    check(jg_open(0, &ctx), "jg_open");

    if (!only || only == 1) {  // (1) C1 writes
        World w{ctx};
        check(jg_keyspace_create(ctx, 128, 1 << 14, &w.ks), "jg_keyspace_create");
        w.make(100, 4, 4, false);
        w.add_keys("key-", 100, 0);
        run("(1) C1 writes: 100 PN-Counter keys x 4 int32 columns, 1M increments", w, [&] {
            Batch b;
            const uint64_t start = rng() % 100;
            for (uint64_t i = 0; i < nq; ++i) b.keys.push("key-" + std::to_string((start + i) % 100)), b.amount.push_back(1 + (int64_t)(rng() % 9));
            return b;
        }, 100, 4, 4, events);
        w.destroy();
    }
    if (!only || only == 2) {  // (2) scaled
        const uint64_t K = 1000000;
        World w{ctx};
        check(jg_keyspace_create(ctx, K, K * 64, &w.ks), "jg_keyspace_create");
        w.make(K, 64, 8, false);
        w.add_keys("key-", K, 0);
        run("(2) scaled: 1M PN-Counter keys x 64 int64 columns, 1M random writes", w, [&] {
            Batch b;
            for (uint64_t i = 0; i < nq; ++i) b.keys.push("key-" + std::to_string(rng() % K)), b.amount.push_back(1 + (int64_t)(rng() % 1000));
            return b;
        }, K, 64, 8, events);
        w.destroy();
    }
    if (!only || only == 3) {  // (3) ORSetWorkload writes
        const uint64_t keys = 10000, batch = 200000, fill_batches = 15;  // bench_names' resident store
        World w{ctx};
        check(jg_keyspace_create(ctx, keys + 16, keys * 64, &w.ks), "jg_keyspace_create");
        w.make(0, 0, 0, true);
        w.add_keys("set", keys, 1);
        std::vector<uint32_t> live(keys, 0);  // names each set holds (Add of a random 5-character string, Clear at 50)
        for (uint64_t f = 0; f < fill_batches; ++f) {
            std::vector<uint32_t> set;
            std::vector<uint8_t> op, is_null, res(batch);
            std::vector<uint64_t> lo, hi;
            Strings names;
            for (uint64_t i = 0; i < batch; ++i) {
                const uint64_t k = rng() % keys;
                const bool clear = live[k] >= 50;  // ORSetWorkload.cs:37-50
                std::string e;
                if (clear) live[k] = 0;
                else {
                    for (int c = 0; c < 5; ++c) e.push_back(kChars[rng() % (sizeof kChars - 1)]);
                    ++live[k];
                }
                set.push_back((uint32_t)k), op.push_back(clear ? 3 : 1), is_null.push_back(0), names.push(e), lo.push_back(rng() | 1), hi.push_back(rng());
            }
            for (Copy& c : w.c)
                check(jg_orset_apply_ops_names(c.ors, batch, set.data(), op.data(), names.off.data(), names.data(), is_null.data(), lo.data(), hi.data(),
                                               res.data(), nullptr, nullptr, nullptr), "jg_orset_apply_ops_names");
        }
        uint64_t na = 0, nr = 0;
        check(jg_orset_size(w.c[0].ors, &na, &nr), "jg_orset_size");
        std::printf("ORSetWorkload shape: %llu sets, store %llu add records\n", (unsigned long long)keys, (unsigned long long)na);
        run("(3) ORSetWorkload writes: 10,000 sets, 200k Adds by (key, element)", w, [&] {
            Batch b;
            b.orset = true;
            for (uint64_t i = 0; i < batch; ++i) {
                std::string e;
                for (int c = 0; c < 5; ++c) e.push_back(kChars[rng() % (sizeof kChars - 1)]);
                b.keys.push("set" + std::to_string(rng() % keys)), b.elems.push(e), b.lo.push_back(rng() | 1), b.hi.push_back(rng());
            }
            return b;
        }, 0, 0, 0, events);
        w.destroy();
    }
    jg_close(ctx);
    return 0;
}
