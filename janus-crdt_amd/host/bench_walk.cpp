// bench_walk.cpp — jg_orset_apply_ops_ords alone, its record walk on the host (jg_orset_set_walk 0, the parent's way)
// and on the device (1), on the ORSetWorkload shape host/bench_names.cpp uses (Add of a random element of a random set;
// a set that has taken 50 Adds is Cleared instead, ORSetWorkload.cs:37-50) and on a mix of Adds and Removes over the
// same sets, whose Removes make the host walk fetch stored runs.
// Four stores hold the same state: two pinned to the host walk (the baseline runs twice per repetition; the distance
// of its two medians is the A/A spread a difference has to exceed), one pinned to the multi-launch device walk and one
// to the device walk with its one-launch form on (jg_orset_set_walk_small 1), which takes every batch
// up to its op cap ("-" past it).  Every repetition applies one fresh batch to all four, in alternating order, and
// compares results and limits; 2 warm-ups, median of 7.
// usage: bench_walk [keys = 10000] [elems = 64]
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
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

double median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

struct Batch {
    std::vector<uint32_t> set, elem;
    std::vector<uint8_t> op;
    std::vector<uint64_t> lo, hi;
};

Batch make(uint64_t keys, uint32_t elems, uint64_t n, bool removes, std::mt19937_64& rng, std::vector<uint8_t>& fill) {
    Batch b;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t k = rng() % keys;
        const bool clear = !removes && fill[k] >= 50;
        if (!removes) fill[k] = clear ? 0 : fill[k] + 1;
        b.set.push_back((uint32_t)k);
        b.elem.push_back((uint32_t)(rng() % elems));
        b.op.push_back(clear ? 3 : removes && (rng() & 1) ? 2 : 1);
        b.lo.push_back(rng() | 1);
        b.hi.push_back(rng());
    }
    return b;
}

struct Out {
    std::vector<uint8_t> res;
    std::vector<uint64_t> al, rl;
};

double apply(jg_orset* s, const Batch& b, Out& o) {
    const uint64_t n = b.set.size();
    o.res.assign(n, 0), o.al.assign(n, 0), o.rl.assign(n, 0);
    const auto t0 = Clock::now();
    check(jg_orset_apply_ops_ords(s, n, b.set.data(), b.elem.data(), b.op.data(), b.lo.data(), b.hi.data(), o.res.data(), o.al.data(), o.rl.data()),
          "jg_orset_apply_ops_ords");
    return ms_since(t0);
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t keys = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 10000;
    const uint32_t elems = argc > 2 ? (uint32_t)std::strtoul(argv[2], nullptr, 10) : 64;
    jg_ctx* ctx;
    check(jg_open(0, &ctx), "jg_open");
    constexpr int kS = 4;
    jg_orset* st[kS];
    const int mode[kS] = {0, 0, 1, 1}, small[kS] = {0, 0, 0, 1};
    const char* name[kS] = {"host", "host", "device", "device, one launch on"};
    for (int k = 0; k < kS; ++k) {
        check(jg_orset_create(ctx, 1 << 20, 1 << 20, &st[k]), "jg_orset_create");
        check(jg_orset_set_walk(st[k], mode[k]), "jg_orset_set_walk");
        check(jg_orset_set_walk_small(st[k], small[k]), "jg_orset_set_walk_small");
    }
    uint64_t ss[6];
    check(jg_orset_walk_small_stats(st[3], ss), "jg_orset_walk_small_stats");
    const uint64_t cap = ss[4];
    std::mt19937_64 rng(20240611);
    std::vector<uint8_t> fill(keys, 0);
    Out o[kS];
    const Batch seed = make(keys, elems, 200000, false, rng, fill);
    for (int k = 0; k < kS; ++k) apply(st[k], seed, o[k]);
    uint64_t na, nr;
    check(jg_orset_size(st[0], &na, &nr), "jg_orset_size");
    std::printf("ORSetWorkload shape: %llu sets x %u elements, store %llu add / %llu tombstone records; one-launch caps: %llu ops, %llu stored tags\n",
                (unsigned long long)keys, elems, (unsigned long long)na, (unsigned long long)nr, (unsigned long long)cap, (unsigned long long)ss[5]);
    const uint64_t sizes[7] = {1, 64, 256, 1024, 2048, 4096, 200000};
    for (int removes = 0; removes < 2; ++removes)
        for (uint64_t n : sizes) {
            std::vector<double> t[kS];
            for (int rep = 0; rep < 9; ++rep) {
                const Batch b = make(keys, elems, n, removes != 0, rng, fill);
                const int first = rep % kS;  // the four ways take turns going first
                double ms[kS];
                for (int j = 0; j < kS; ++j) {
                    const int k = (first + j) % kS;
                    ms[k] = apply(st[k], b, o[k]);
                }
                for (int k = 1; k < kS; ++k)
                    if (o[k].res != o[0].res || o[k].al != o[0].al || o[k].rl != o[0].rl) {
                        std::fprintf(stderr, "mismatch: store %d against store 0 at %llu ops\n", k, (unsigned long long)n);
                        return 2;
                    }
                if (rep >= 2)
                    for (int k = 0; k < kS; ++k) t[k].push_back(ms[k]);
            }
            const double m1 = median(t[0]), m2 = median(t[1]), dev = median(t[2]), one = median(t[3]), base = std::min(m1, m2),
                         spread = std::abs(m1 - m2);
            std::printf("%s, %llu ops: host walk %.3f / %.3f ms (A/A spread %.3f ms); device walk %.3f ms = %.2fx the host walk: %s; ",
                        removes ? "Add/Remove mix" : "ORSetWorkload", (unsigned long long)n, m1, m2, spread, dev, dev / base,
                        dev <= base + spread ? "within the bar" : "MISSES the bar");
            if (n <= cap)
                std::printf("one launch %.3f ms = %.2fx the host walk: %s\n", one, one / base, one <= base + spread ? "within the bar" : "MISSES the bar");
            else
                std::printf("one launch - (past its cap: multi-launch %.3f ms)\n", one);
        }
    uint64_t ws[4];
    for (int k : {0, 2, 3}) {
        check(jg_orset_walk_stats(st[k], ws), "jg_orset_walk_stats");
        check(jg_orset_walk_small_stats(st[k], ss), "jg_orset_walk_small_stats");
        std::printf("store pinned to %s: %llu device batches, %llu host batches, %llu device ops, %llu run bytes to the host; %llu batches of %llu ops "
                    "in one launch, %llu over the stored-tag budget\n", name[k], (unsigned long long)ws[0], (unsigned long long)ws[1],
                    (unsigned long long)ws[2], (unsigned long long)ws[3], (unsigned long long)ss[0], (unsigned long long)ss[1], (unsigned long long)ss[2]);
    }
    uint64_t a[kS], r[kS];
    for (int k = 0; k < kS; ++k) check(jg_orset_size(st[k], &a[k], &r[k]), "jg_orset_size");
    for (int k = 1; k < kS; ++k)
        if (a[k] != a[0] || r[k] != r[0]) {
            std::fprintf(stderr, "mismatch: the stores' sizes differ at the end\n");
            return 2;
        }
    for (int k = 0; k < kS; ++k) check(jg_orset_destroy(st[k]), "jg_orset_destroy");
    check(jg_close(ctx), "jg_close");
    return 0;
}
