// host/bench_query.cpp — client reads by key name in one call (jg_node_query_keys, csrc/query.hip)
// beside the parent's way: jg_keyspace_lookup -> one thread of unordered_map<guid, (type, idx)> -> jg_pnc_values /
// jg_orset_contains_names.
//   (1) C1 reads: 100 PN-Counter keys, 1M "gs" reads per call, keys round-robin from a random start (PNCWorkload.cs:32-92)
//   (2) scaled: 1M PN-Counter keys x 64 int64 columns, 1M uniformly random reads
//   (3) ORSetWorkload reads: bench_names' resident shape (10,000 sets), 1M Contains by (key, element), half of them members
// Wall time of the calls a caller makes; 2 warm-ups, median of 7, the two ways alternating.  The parent's way runs twice
// per repetition, and the distance of its two medians is the A/A spread a difference has to exceed.  Every run's outputs
// are compared between the two ways.
// `--events`: one repetition per shape with JANUS_TRACE_QUERY set, so the library reports the upload, the launches and
// the copies out by hipEvents on stderr; the bytes on the host link are printed beside them.
// usage: bench_query [--events] [--shape 1|2|3]
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

struct Answers {
    std::vector<int64_t> value;
    std::vector<uint8_t> status;
    explicit Answers(uint64_t n) : value(n), status(n) {}
};

struct World {
    jg_ctx* ctx;
    jg_keyspace* ks = nullptr;
    jg_pnc* pnc = nullptr;
    jg_orset* ors = nullptr;
    jg_node* node = nullptr;
    UidMap uids;
    // n keys named prefix + index, guid from the index, registered as `type` with idx = index
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
        check(jg_node_register(node, n, g.data(), t.data(), idx.data()), "jg_node_register");
    }
};

// the parent's way: three steps, a host round trip between each
double parent_way(World& w, const Strings& keys, const Strings* elems, Answers& a) {
    const uint64_t n = keys.n();
    const auto t0 = Clock::now();
    std::vector<jg_guid> guid(n);
    std::vector<uint8_t> found(n);
    check(jg_keyspace_lookup(w.ks, n, keys.off.data(), keys.data(), guid.data(), found.data()), "jg_keyspace_lookup");
    std::vector<uint32_t> idx(n);
    bool orset = false;
    for (uint64_t i = 0; i < n; ++i) {
        const auto it = found[i] ? w.uids.find(guid[i]) : w.uids.end();
        require(it != w.uids.end(), "every benchmark key resolves");
        idx[i] = it->second.idx;
        orset = it->second.type == 1;
    }
    if (!orset) {
        check(jg_pnc_values(w.pnc, idx.data(), n, a.value.data(), a.status.data()), "jg_pnc_values");
        for (uint64_t i = 0; i < n; ++i) a.status[i] = a.status[i] ? JG_Q_OVERFLOW : JG_Q_OK;
    } else {
        std::vector<uint8_t> is_null(n, 0), out(n);
        check(jg_orset_contains_names(w.ors, n, idx.data(), elems->off.data(), elems->data(), is_null.data(), out.data()), "jg_orset_contains_names");
        for (uint64_t i = 0; i < n; ++i) a.value[i] = out[i], a.status[i] = JG_Q_OK;
    }
    return ms_since(t0);
}

double by_key(World& w, const Strings& keys, const Strings* elems, const std::vector<uint8_t>& flag, Answers& a) {
    const uint64_t n = keys.n();
    const auto t0 = Clock::now();
    std::vector<uint8_t> kind(n);
    check(jg_node_query_keys(w.node, w.ks, n, keys.off.data(), keys.data(), elems ? elems->off.data() : nullptr, elems ? elems->data() : nullptr,
                             elems ? flag.data() : nullptr, a.value.data(), a.status.data(), kind.data(), nullptr), "jg_node_query_keys");
    return ms_since(t0);
}

void run(const char* what, World& w, const Strings& keys, const Strings* elems, bool events) {
    const uint64_t n = keys.n();
    const int warm = events ? 1 : 2, reps = events ? 1 : 7;
    const std::vector<uint8_t> flag(n, 1);
    Answers ak(n), a1(n), a2(n);
    std::vector<double> t, b1, b2;
    for (int r = 0; r < warm + reps; ++r) {
        const double x = parent_way(w, keys, elems, a1);
        const double y = by_key(w, keys, elems, flag, ak);
        const double z = parent_way(w, keys, elems, a2);
        require(ak.value == a1.value && ak.status == a1.status && a1.value == a2.value && a1.status == a2.status, what);
        if (r >= warm) t.push_back(y), b1.push_back(x), b2.push_back(z);
    }
    const double m = median(t), m1 = median(b1), m2 = median(b2), base = std::min(m1, m2), spread = std::abs(m1 - m2);
    std::printf("%s: by key %.3f ms; parent's way %.3f / %.3f ms (A/A spread %.3f ms = %.1f%%); by key is %.2fx the parent's way: %s\n", what, m, m1, m2,
                spread, 100 * spread / base, m / base, m <= std::max(m1, m2) + spread ? "within the bar" : "SLOWER than the parent's way");
    const uint64_t up = keys.bytes.size() + (n + 1) * 8 + (elems ? elems->bytes.size() + (n + 1) * 8 + n : 0), down = n * 10;
    std::printf("    %llu reads, %llu answers nonzero; %llu bytes up + %llu bytes down = %.4f ms on the host link at 57 GB/s\n", (unsigned long long)n,
                (unsigned long long)std::count_if(ak.value.begin(), ak.value.end(), [](int64_t v) { return v != 0; }), (unsigned long long)up,
                (unsigned long long)down, (up + down) / 57e9 * 1e3);
}

}  // namespace

int main(int argc, char** argv) {
    bool events = false;
    int only = 0;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--events")) events = true;
        else if (!std::strcmp(argv[i], "--shape") && i + 1 < argc) only = std::atoi(argv[++i]);
    }
    if (events) setenv("JANUS_TRACE_QUERY", "1", 1);  // the library latches it at its first call
    const uint64_t nq = 1000000;
    std::mt19937_64 rng(2025);
    jg_ctx* ctx = nullptr;
    check(jg_open(0, &ctx), "jg_open");

    if (!only || only == 1) {  // (1) C1 reads
        World w{ctx};
        check(jg_keyspace_create(ctx, 128, 1 << 14, &w.ks), "jg_keyspace_create");
        check(jg_pnc_create(ctx, 100, 4, 4, &w.pnc), "jg_pnc_create");
        check(jg_synth_pnc_store(w.pnc, 7), "jg_synth_pnc_store");
        check(jg_node_create(w.pnc, nullptr, &w.node), "jg_node_create");
        w.add_keys("counter", 100, 0);
        Strings q;
        const uint64_t start = rng() % 100;
        for (uint64_t i = 0; i < nq; ++i) q.push("counter" + std::to_string((start + i) % 100));
        run("(1) C1 reads: 100 PN-Counter keys, 1M reads", w, q, nullptr, events);
        jg_node_destroy(w.node), jg_pnc_destroy(w.pnc), jg_keyspace_destroy(w.ks);
    }
    if (!only || only == 2) {  // (2) scaled
        const uint64_t K = 1000000;
        World w{ctx};
        check(jg_keyspace_create(ctx, K, K * 64, &w.ks), "jg_keyspace_create");
        check(jg_pnc_create(ctx, K, 64, 8, &w.pnc), "jg_pnc_create");
        check(jg_synth_pnc_store(w.pnc, 8), "jg_synth_pnc_store");
        check(jg_node_create(w.pnc, nullptr, &w.node), "jg_node_create");
        w.add_keys("key-", K, 0);
        Strings q;
        for (uint64_t i = 0; i < nq; ++i) q.push("key-" + std::to_string(rng() % K));
        run("(2) scaled: 1M PN-Counter keys x 64 int64 columns, 1M random reads", w, q, nullptr, events);
        jg_node_destroy(w.node), jg_pnc_destroy(w.pnc), jg_keyspace_destroy(w.ks);
    }
    if (!only || only == 3) {  // (3) ORSetWorkload reads
        const uint64_t keys = 10000, batch = 200000, fill_batches = 15;  // bench_names' store when it measures Contains
        World w{ctx};
        check(jg_keyspace_create(ctx, keys + 16, keys * 64, &w.ks), "jg_keyspace_create");
        check(jg_orset_create(ctx, 0, 0, &w.ors), "jg_orset_create");
        check(jg_node_create(nullptr, w.ors, &w.node), "jg_node_create");
        w.add_keys("set", keys, 1);
        std::vector<std::vector<std::string>> live(keys);  // the names each set holds (Add of a random 5-character string, Clear at 50)
        for (uint64_t b = 0; b < fill_batches; ++b) {
            std::vector<uint32_t> set;
            std::vector<uint8_t> op, is_null, res;
            std::vector<uint64_t> lo, hi;
            Strings names;
            for (uint64_t i = 0; i < batch; ++i) {
                const uint64_t k = rng() % keys;
                const bool clear = live[k].size() >= 50;  // ORSetWorkload.cs:37-50
                std::string e;
                if (clear) live[k].clear();
                else {
                    for (int c = 0; c < 5; ++c) e.push_back(kChars[rng() % (sizeof kChars - 1)]);
                    live[k].push_back(e);
                }
                set.push_back((uint32_t)k), op.push_back(clear ? 3 : 1), is_null.push_back(0), names.push(e), lo.push_back(rng() | 1), hi.push_back(rng());
            }
            res.resize(batch);
            check(jg_orset_apply_ops_names(w.ors, batch, set.data(), op.data(), names.off.data(), names.data(), is_null.data(), lo.data(), hi.data(),
                                           res.data(), nullptr, nullptr, nullptr), "jg_orset_apply_ops_names");
        }
        uint64_t na = 0, nr = 0;
        check(jg_orset_size(w.ors, &na, &nr), "jg_orset_size");
        std::printf("ORSetWorkload shape: %llu sets, store %llu add records\n", (unsigned long long)keys, (unsigned long long)na);
        Strings q, e;
        for (uint64_t i = 0; i < nq; ++i) {
            const uint64_t k = rng() % keys;
            q.push("set" + std::to_string(k));
            if (i % 2 == 0 && !live[k].empty()) e.push(live[k][rng() % live[k].size()]);
            else {
                std::string s;
                for (int c = 0; c < 5; ++c) s.push_back(kChars[rng() % (sizeof kChars - 1)]);
                e.push(s);
            }
        }
        run("(3) ORSetWorkload reads: 10,000 sets, 1M Contains by (key, element)", w, q, &e, events);
        jg_node_destroy(w.node), jg_orset_destroy(w.ors), jg_keyspace_destroy(w.ks);
    }
    jg_close(ctx);
    return 0;
}
