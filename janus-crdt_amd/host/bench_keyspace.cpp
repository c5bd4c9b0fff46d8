// host/bench_keyspace.cpp — the key-space set's four shapes on the device (jg_tpset_*, csrc/tpset.hip, tpset_encode.hip; (e): keyspace.hip) beside the same
// work on host/tpset_ref.hpp with one thread (a port of the reference's decode + UnionWith, as README's other CPU
// baselines are).  K entries of the C5 key shape: 11-byte key, NUL, 36-byte Guid.
//   (a) steady creation: a resident set of K receives one full state of K + 1 entries; also with the serial parser
//   (b) cold: an empty set receives K
//   (c) 1000 small states of 0-20 entries in one call
//   (d) Encode of the K + 1 entries
//   (e) jg_keyspace_receive of the K + 1 state into a key space that knows K keys: one new key learnt
// Device times are hipEvent seconds the library reports (jg_tpset_last_stats: the call's kernels, the upload and the
// copy out excluded; the host reads between launches included); 2 warm-ups, median of 7.  (a) and (b) build their set
// anew for every run, so that each timed merge meets the state the shape names; (e) is wall time of the entry point
// a key-space host calls, jg_keyspace_receive (upload, merge, OnNext).  The encoded bytes and the
// sizes are checked against the restatement on every run.
// usage: bench_keyspace [K = 1000000] [--no-serial]
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "janus_gpu.h"
#include "tpset_ref.hpp"

namespace {

using Clock = std::chrono::steady_clock;
double since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

void check(int rc, const char* what) {
    if (rc == JG_OK) return;
    char buf[512];
    jg_last_error(buf, sizeof buf);
    std::fprintf(stderr, "%s failed: [%d] %s\n", what, rc, buf);
    std::exit(1);
}

std::string entry_wire(uint64_t i) {  // "key0000001\u0000xxxxxxxx-xxxx-4xxx-8xxx-xxxxxxxxxxxx"
    char b[96];
    std::snprintf(b, sizeof b, "\"key%08llu\\u0000%08llx-%04llx-4%03llx-8%03llx-%012llx\"", (unsigned long long)i,
                  (unsigned long long)(i * 2654435761ull % (1ull << 32)), (unsigned long long)(i % 65536), (unsigned long long)(i % 4096),
                  (unsigned long long)(i * 7 % 4096), (unsigned long long)(i * 1000003ull % (1ull << 48)));
    return b;
}

std::string message(uint64_t first, uint64_t n) {
    std::string m = "{\"addSet\":[";
    for (uint64_t i = 0; i < n; ++i) {
        if (i) m.push_back(',');
        m += entry_wire(first + i);
    }
    return m + "],\"removeSet\":[]}";
}

struct Batch {
    std::vector<uint64_t> off{0};
    std::string bytes;
    void add(const std::string& m) {
        bytes += m;
        off.push_back(bytes.size());
    }
    uint64_t n() const { return off.size() - 1; }
};

double median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

// merges `b` reps times after `warm` warm-ups; the median device seconds and the last call's figures
double run_merge(jg_tpset* s, const Batch& b, uint32_t mode, int warm, int reps, jg_tpset_stats* last) {
    std::vector<double> t;
    for (int r = 0; r < warm + reps; ++r) {
        uint64_t bad;
        uint8_t partial;
        check(jg_tpset_merge_json(s, b.n(), b.off.data(), reinterpret_cast<const uint8_t*>(b.bytes.data()), mode, &bad, &partial), "jg_tpset_merge_json");
        check(jg_tpset_last_stats(s, last), "jg_tpset_last_stats");
        if (r >= warm) t.push_back(last->device_s);
    }
    return median(t);
}

double cpu_merge(janus::ref::TPSet& set, const Batch& b) {
    const auto t0 = Clock::now();
    for (uint64_t m = 0; m < b.n(); ++m)
        if (janus::ref::MergeJson(set, std::string_view(b.bytes).substr(b.off[m], b.off[m + 1] - b.off[m])) != 0) std::exit(2);
    return since(t0);
}

void report(const char* shape, double dev_s, uint64_t bytes, const jg_tpset_stats& st, double cpu_s) {
    std::printf("%-34s device %9.3f ms  %7.2f GB/s  parser %s  | tpset_ref.hpp 1 thread %10.1f ms  (x%.0f)\n", shape, dev_s * 1e3, bytes / dev_s / 1e9,
                st.msgs_serial == 0 ? "scanner" : st.msgs_parallel == 0 ? "serial" : "both", cpu_s * 1e3, cpu_s / dev_s);
    std::fflush(stdout);
}

void same_set(jg_tpset* s, const janus::ref::TPSet& ref, const char* where) {
    uint64_t na, nr, nb, len = 0;
    check(jg_tpset_size(s, &na, &nr, &nb), "jg_tpset_size");
    check(jg_tpset_encode_json(s, &len, nullptr, 0), "jg_tpset_encode_json");
    std::string wire(len, '\0');
    check(jg_tpset_encode_json(s, &len, reinterpret_cast<uint8_t*>(wire.data()), len), "jg_tpset_encode_json");
    if (na != ref.addSet().Count() || nr != ref.removeSet().Count() || wire != ref.Encode()) {
        std::fprintf(stderr, "PARITY FAILED %s\n", where);
        std::exit(3);
    }
}

}  // namespace

int main(int argc, char** argv) {
    uint64_t K = 1000000;
    bool serial = true;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--no-serial")) serial = false;
        else K = std::strtoull(argv[i], nullptr, 10);
    }
    Batch full, full1, small;
    full.add(message(0, K));
    full1.add(message(0, K + 1));
    uint64_t x = 12345;
    for (int i = 0; i < 1000; ++i) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        small.add(message((x >> 33) % (K > 20 ? K - 20 : 1), (x >> 20) % 21));
    }
    std::printf("K = %llu entries, full state %.1f MB\n", (unsigned long long)K, full1.bytes.size() / 1e6);

    jg_ctx* ctx;
    check(jg_open(0, &ctx), "jg_open");
    const uint64_t cap_s = K + 1024, cap_b = 64 * cap_s;
    jg_tpset_stats st{};

    // (a) steady creation: every run a set that holds K, then the timed state of K + 1 (one new string)
    jg_tpset* s = nullptr;
    janus::ref::TPSet ref;
    cpu_merge(ref, full);
    const double a_cpu = cpu_merge(ref, full1);
    auto steady = [&](uint32_t mode, int warm, int reps) {
        std::vector<double> t;
        for (int r = 0; r < warm + reps; ++r) {
            if (s) check(jg_tpset_destroy(s), "jg_tpset_destroy");
            check(jg_tpset_create(ctx, cap_s, cap_b, &s), "jg_tpset_create");
            run_merge(s, full, 0, 0, 1, &st);
            const double d = run_merge(s, full1, mode, 0, 1, &st);
            if (st.strings_new != 1) std::exit(4);
            if (r >= warm) t.push_back(d);
        }
        return median(t);
    };
    const double a_dev = steady(0, 2, 7);
    report("(a) steady, K resident + state K+1", a_dev, full1.bytes.size(), st, a_cpu);
    same_set(s, ref, "(a)");
    if (serial) {
        const double a1 = steady(1, 0, 1);
        report("(a) the same, mode 1", a1, full1.bytes.size(), st, a_cpu);
    }
    // (d) encode
    {
        uint64_t len = 0;
        check(jg_tpset_encode_json(s, &len, nullptr, 0), "jg_tpset_encode_json");
        std::string wire(len, '\0');
        std::vector<double> t;
        for (int r = 0; r < 9; ++r) {
            check(jg_tpset_encode_json(s, &len, reinterpret_cast<uint8_t*>(wire.data()), len), "jg_tpset_encode_json");
            check(jg_tpset_last_stats(s, &st), "jg_tpset_last_stats");
            if (r >= 2) t.push_back(st.encode_s);
        }
        const auto t0 = Clock::now();
        const std::string cpu = ref.Encode();
        const double d_cpu = since(t0), d_dev = median(t);
        if (cpu != wire) return 3;
        std::printf("%-34s device %9.3f ms  %7.2f GB/s  staged %llu B      | tpset_ref.hpp 1 thread %10.1f ms  (x%.0f)\n", "(d) Encode of K+1 entries", d_dev * 1e3,
                    len / d_dev / 1e9, (unsigned long long)st.stage_bytes, d_cpu * 1e3, d_cpu / d_dev);
    }
    check(jg_tpset_destroy(s), "jg_tpset_destroy");

    // (b) cold: a fresh set per run
    {
        std::vector<double> t;
        for (int r = 0; r < 9; ++r) {
            check(jg_tpset_create(ctx, cap_s, cap_b, &s), "jg_tpset_create");
            const double d = run_merge(s, full, 0, 0, 1, &st);
            if (r >= 2) t.push_back(d);
            check(jg_tpset_destroy(s), "jg_tpset_destroy");
        }
        janus::ref::TPSet cold;
        report("(b) cold, empty set receives K", median(t), full.bytes.size(), st, cpu_merge(cold, full));
    }
    // (c) 1000 small states in one call
    {
        check(jg_tpset_create(ctx, cap_s, cap_b, &s), "jg_tpset_create");
        janus::ref::TPSet sm;
        const double c_cpu = cpu_merge(sm, small);
        const double c_dev = run_merge(s, small, 0, 2, 7, &st);
        report("(c) 1000 states of 0-20 entries", c_dev, small.bytes.size(), st, c_cpu);
        same_set(s, sm, "(c)");
        const double c1 = run_merge(s, small, 1, 2, 7, &st);
        report("(c) the same, mode 1", c1, small.bytes.size(), st, c_cpu);
        check(jg_tpset_destroy(s), "jg_tpset_destroy");
    }
    // (e) the entry point a key-space host calls: Merge + OnNext of the K + 1 state where K keys are known
    {
        std::vector<double> t;
        janus::ref::KeySpace kref;
        if (kref.Receive(full.bytes) != 0) return 2;
        const auto c0 = Clock::now();
        if (kref.Receive(full1.bytes) != 0) return 2;
        const double e_cpu = since(c0);
        uint64_t n_new = 0, bad;
        uint8_t partial;
        for (int r = 0; r < 5; ++r) {
            jg_keyspace* ks;
            check(jg_keyspace_create(ctx, cap_s, cap_b, &ks), "jg_keyspace_create");
            check(jg_keyspace_receive(ks, 1, full.off.data(), reinterpret_cast<const uint8_t*>(full.bytes.data()), 0, &bad, &partial, &n_new), "jg_keyspace_receive");
            if (n_new != K) return 3;
            const auto t0 = Clock::now();
            check(jg_keyspace_receive(ks, 1, full1.off.data(), reinterpret_cast<const uint8_t*>(full1.bytes.data()), 0, &bad, &partial, &n_new), "jg_keyspace_receive");
            if (r >= 1) t.push_back(since(t0));
            if (n_new != 1 || kref.journal().size() != K + 1) return 3;
            check(jg_keyspace_destroy(ks), "jg_keyspace_destroy");
        }
        const double e = median(t);
        std::printf("%-34s wall   %9.3f ms  %7.2f GB/s  upload + merge + OnNext   | tpset_ref.hpp 1 thread %10.1f ms  (x%.0f)\n", "(e) jg_keyspace_receive, K known", e * 1e3,
                    full1.bytes.size() / e / 1e9, e_cpu * 1e3, e_cpu / e);
    }
    check(jg_close(ctx), "jg_close");
    std::printf("PARITY OK\n");
    return 0;
}
