// host/bench_names.cpp — the OR-Set by element name (jg_orset_*_names, csrc/orset_names.hip) beside the caller-side
// dictionaries it replaces, on the ORSetWorkload shape host/bench_submit.cpp uses (Add of a random 5-character string
// with a fresh tag, Clear once a set holds 50 elements, over `keys` sets).
//   (a) 1M Contains: jg_orset_contains_names, against one thread of unordered_map<string, uint32_t> lookups +
//       jg_orset_contains
//   (b) one batch of 200k ops: jg_orset_apply_ops_names, against host interning + jg_orset_names_sync +
//       jg_orset_apply_ops_ords
//   (c) LookupAll of every set as strings: jg_orset_lookup_all_names (size query + fill), against jg_orset_lookup_all
//       (size query + fill) + host id -> string
// Wall time of the calls a caller makes; 2 warm-ups, median of 7, the two ways alternating.  The baseline runs twice
// per repetition (on two stores for (b), whose batches change the state), and the distance of those two medians is
// the A/A spread a difference has to exceed.  Every run's outputs are compared between the two ways.
// `--events`: (b) only, with JANUS_TRACE_APPLY set, so the library reports the device time of the resolve / intern
// launches (hipEvents) on stderr, apart from the record walk both ways share.
// usage: bench_names [keys = 10000] [--events]
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

struct Ops {  // one batch, names packed as the by-name calls take them
    std::vector<uint32_t> set;
    std::vector<uint8_t> op, is_null;
    std::vector<uint64_t> off{0}, lo, hi;
    std::string bytes;
    uint64_t n() const { return set.size(); }
    std::string_view name(uint64_t i) const { return std::string_view(bytes).substr(off[i], off[i + 1] - off[i]); }
};

Ops make_ops(uint64_t keys, uint64_t n, std::mt19937_64& rng, std::vector<uint8_t>& fill) {
    Ops o;
    while (o.n() < n) {
        const uint64_t k = rng() % keys;
        const bool clear = fill[k] >= 50;  // ORSetWorkload.cs:37-50
        fill[k] = clear ? 0 : fill[k] + 1;
        o.set.push_back((uint32_t)k);
        o.op.push_back(clear ? 3 : 1);
        o.is_null.push_back(0);
        if (!clear)
            for (int c = 0; c < 5; ++c) o.bytes.push_back(kChars[rng() % (sizeof kChars - 1)]);
        o.off.push_back(o.bytes.size());
        o.lo.push_back(rng() | 1);
        o.hi.push_back(rng());
    }
    return o;
}

// The caller-side tables of the id-taking surface (GpuStableStore's SetKey, INTEGRATION.md §3c's GpuORSet).
struct HostNames {
    struct Set {
        std::unordered_map<std::string, uint32_t> ids;  // live element -> id
        std::vector<std::string> names;                 // id -> element, every id ever issued
    };
    std::vector<Set> sets;
    std::vector<uint32_t> clears;  // Clears each set has seen
    explicit HostNames(uint64_t keys) : sets(keys), clears(keys, 0) {}
};

struct Result {
    std::vector<uint8_t> res;
    std::vector<uint64_t> al, rl;
};

// The parent's way: intern on the host, tell the table, apply by id.  As GpuStableStore does, a set Cleared in the
// batch is told so once, and only the names interned after its last Clear are registered (the earlier ones are
// dead by the batch's end and carry no records).
void apply_by_id(jg_orset* s, HostNames& H, const Ops& o, Result& r) {
    const uint64_t n = o.n();
    std::vector<uint32_t> elem(n), sset, snext, nset, nid;
    std::vector<uint8_t> sclr;
    std::vector<uint64_t> noff{0};
    std::string nbytes;
    std::unordered_map<uint32_t, uint32_t> touched;  // set -> index in sset
    struct New { uint32_t set, id, clears; uint64_t op; };
    std::vector<New> fresh;
    for (uint64_t i = 0; i < n; ++i) {
        HostNames::Set& S = H.sets[o.set[i]];
        auto touch = [&]() -> uint32_t {
            auto it = touched.find(o.set[i]);
            if (it != touched.end()) return it->second;
            sset.push_back(o.set[i]), snext.push_back(0), sclr.push_back(0);
            return touched.emplace(o.set[i], (uint32_t)sset.size() - 1).first->second;
        };
        if (o.op[i] == 3) {
            S.ids.clear();
            sclr[touch()] = 1;
            elem[i] = 0;
            ++H.clears[o.set[i]];
            continue;
        }
        const std::string e(o.name(i));
        auto it = S.ids.find(e);
        if (it != S.ids.end()) { elem[i] = it->second; continue; }
        if (o.op[i] == 2) { elem[i] = JG_NULL_ELEM - 1; continue; }
        const uint32_t id = (uint32_t)S.names.size();
        S.ids.emplace(e, id);
        S.names.push_back(e);
        elem[i] = id;
        touch();
        fresh.push_back(New{o.set[i], id, H.clears[o.set[i]], i});
    }
    for (size_t k = 0; k < sset.size(); ++k) snext[k] = (uint32_t)H.sets[sset[k]].names.size();
    for (const New& f : fresh) {
        if (f.clears != H.clears[f.set]) continue;  // interned before a Clear of this batch: dead by its end
        nset.push_back(f.set), nid.push_back(f.id);
        nbytes += o.name(f.op);
        noff.push_back(nbytes.size());
    }
    check(jg_orset_names_sync(s, sset.size(), sset.data(), snext.data(), sclr.data(), nset.size(), nset.data(), nid.data(), noff.data(),
                              reinterpret_cast<const uint8_t*>(nbytes.data())), "jg_orset_names_sync");
    r.res.assign(n, 0), r.al.assign(n, 0), r.rl.assign(n, 0);
    check(jg_orset_apply_ops_ords(s, n, o.set.data(), elem.data(), o.op.data(), o.lo.data(), o.hi.data(), r.res.data(), r.al.data(), r.rl.data()),
          "jg_orset_apply_ops_ords");
}

void apply_by_name(jg_orset* s, const Ops& o, Result& r) {
    const uint64_t n = o.n();
    r.res.assign(n, 0), r.al.assign(n, 0), r.rl.assign(n, 0);
    check(jg_orset_apply_ops_names(s, n, o.set.data(), o.op.data(), o.off.data(), reinterpret_cast<const uint8_t*>(o.bytes.data()), o.is_null.data(),
                                   o.lo.data(), o.hi.data(), r.res.data(), nullptr, r.al.data(), r.rl.data()), "jg_orset_apply_ops_names");
}

void report(const char* what, const std::vector<double>& name, const std::vector<double>& b1, const std::vector<double>& b2) {
    const double m = median(name), m1 = median(b1), m2 = median(b2), base = std::min(m1, m2), spread = std::abs(m1 - m2);
    std::printf("%s: by name %.3f ms; parent's way %.3f / %.3f ms (A/A spread %.3f ms = %.1f%%); by name is %.2fx the parent's way: %s\n", what, m, m1,
                m2, spread, 100 * spread / base, m / base, m <= std::max(m1, m2) + spread ? "within the bar" : "SLOWER than the parent's way");
}

}  // namespace

int main(int argc, char** argv) {
    uint64_t keys = 10000;
    bool events = false;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--events")) events = true;
        else keys = std::strtoull(argv[i], nullptr, 10);
    }
    if (events) setenv("JANUS_TRACE_APPLY", "1", 1);
    const int warm = 2, reps = events ? 1 : 7;
    const uint64_t batch = 200000, fill_batches = 6;
    jg_ctx* ctx = nullptr;
    check(jg_open(0, &ctx), "jg_open");
    jg_orset *sn = nullptr, *t1 = nullptr, *t2 = nullptr;
    check(jg_orset_create(ctx, 0, 0, &sn), "jg_orset_create");
    check(jg_orset_create(ctx, 0, 0, &t1), "jg_orset_create");
    check(jg_orset_create(ctx, 0, 0, &t2), "jg_orset_create");
    HostNames h1(keys), h2(keys);
    std::mt19937_64 rng(2024);
    std::vector<uint8_t> fill(keys, 0);
    Result rn, r1, r2;

    // the stores filled to the workload's steady state, then (b): each repetition applies a fresh batch three times
    std::vector<double> tn, tb1, tb2;
    uint64_t name_bytes = 0;
    for (uint64_t k = 0; k < fill_batches + warm + reps; ++k) {
        const Ops o = make_ops(keys, batch, rng, fill);
        name_bytes = o.bytes.size();
        const bool first = k % 2 == 0;  // alternate which baseline store goes first
        auto t0 = Clock::now();
        apply_by_id(first ? t1 : t2, first ? h1 : h2, o, first ? r1 : r2);
        const double a = ms_since(t0);
        t0 = Clock::now();
        apply_by_name(sn, o, rn);
        const double b = ms_since(t0);
        t0 = Clock::now();
        apply_by_id(first ? t2 : t1, first ? h2 : h1, o, first ? r2 : r1);
        const double c = ms_since(t0);
        require(rn.res == r1.res && rn.al == r1.al && rn.rl == r1.rl && r1.res == r2.res && r1.al == r2.al, "(b) results / ord limits");
        if (k >= fill_batches + warm) tn.push_back(b), tb1.push_back(first ? a : c), tb2.push_back(first ? c : a);
    }
    uint64_t na = 0, nr = 0, ma = 0, mr = 0;
    check(jg_orset_size(sn, &na, &nr), "jg_orset_size");
    check(jg_orset_size(t1, &ma, &mr), "jg_orset_size");
    require(na == ma && nr == mr, "(b) store sizes");
    std::printf("ORSetWorkload shape: %llu sets, batches of %llu ops, store %llu add records\n", (unsigned long long)keys,
                (unsigned long long)batch, (unsigned long long)na);
    if (events) {
        std::printf("(b) with --events: one batch carries %llu name bytes = %.4f ms on the host link at 57 GB/s (the library's lines above give the "
                    "launches)\n", (unsigned long long)name_bytes, name_bytes / 57e9 * 1e3);
        return 0;
    }
    report("(b) 200k-op batch", tn, tb1, tb2);
    std::printf("    one batch carries %llu name bytes = %.4f ms on the host link at 57 GB/s\n", (unsigned long long)name_bytes, name_bytes / 57e9 * 1e3);

    // (a) 1M Contains: half the names are live members, half random strings
    {
        const uint64_t nq = 1000000;
        Ops q;
        for (uint64_t i = 0; i < nq; ++i) {
            const uint32_t k = (uint32_t)(rng() % keys);
            const auto& S = h1.sets[k];
            q.set.push_back(k);
            q.is_null.push_back(0);
            if (i % 2 == 0 && !S.ids.empty()) q.bytes += S.names[S.names.size() - 1 - rng() % S.ids.size()];
            else
                for (int c = 0; c < 5; ++c) q.bytes.push_back(kChars[rng() % (sizeof kChars - 1)]);
            q.off.push_back(q.bytes.size());
        }
        std::vector<uint8_t> on(nq), ob(nq);
        std::vector<uint32_t> elem(nq);
        auto base = [&] {
            const auto t0 = Clock::now();
            for (uint64_t i = 0; i < nq; ++i) {
                const auto& ids = h1.sets[q.set[i]].ids;
                const auto it = ids.find(std::string(q.name(i)));
                elem[i] = it == ids.end() ? JG_NULL_ELEM - 1 : it->second;
            }
            check(jg_orset_contains(t1, q.set.data(), elem.data(), nq, ob.data()), "jg_orset_contains");
            return ms_since(t0);
        };
        std::vector<double> a, b1, b2;
        for (int r = 0; r < warm + reps; ++r) {
            const double x = base();
            const auto t0 = Clock::now();
            check(jg_orset_contains_names(sn, nq, q.set.data(), q.off.data(), reinterpret_cast<const uint8_t*>(q.bytes.data()), q.is_null.data(),
                                          on.data()), "jg_orset_contains_names");
            const double y = ms_since(t0);
            const double z = base();
            require(on == ob, "(a) Contains");
            if (r >= warm) a.push_back(y), b1.push_back(x), b2.push_back(z);
        }
        const uint64_t hits = std::count(on.begin(), on.end(), 1);
        report("(a) 1M Contains", a, b1, b2);
        std::printf("    %llu present; %llu name bytes = %.4f ms on the host link at 57 GB/s\n", (unsigned long long)hits,
                    (unsigned long long)q.bytes.size(), q.bytes.size() / 57e9 * 1e3);
    }

    // (c) LookupAll of every set, as strings
    {
        std::vector<uint32_t> sets(keys);
        for (uint64_t k = 0; k < keys; ++k) sets[k] = (uint32_t)k;
        std::vector<uint64_t> off(keys + 1), noff, boff(keys + 1), bnoff;
        std::vector<uint8_t> bytes, isn, bbytes;
        std::vector<uint32_t> ids;
        auto by_name = [&] {
            const auto t0 = Clock::now();
            uint64_t nb = 0;
            check(jg_orset_lookup_all_names(sn, keys, sets.data(), off.data(), &nb, nullptr, nullptr, nullptr, nullptr, 0, 0), "lookup_all_names (size)");
            noff.resize(off[keys] + 1), bytes.resize(nb + 1), isn.resize(off[keys] + 1);
            check(jg_orset_lookup_all_names(sn, keys, sets.data(), off.data(), &nb, noff.data(), bytes.data(), isn.data(), nullptr, off[keys], nb),
                  "lookup_all_names");
            bytes.resize(nb);
            return ms_since(t0);
        };
        auto base = [&] {
            const auto t0 = Clock::now();
            check(jg_orset_lookup_all(t1, keys, sets.data(), boff.data(), nullptr, 0), "lookup_all (size)");
            ids.resize(boff[keys] + 1);
            check(jg_orset_lookup_all(t1, keys, sets.data(), boff.data(), ids.data(), boff[keys]), "lookup_all");
            bbytes.clear();
            bnoff.assign(1, 0);
            for (uint64_t k = 0; k < keys; ++k)
                for (uint64_t m = boff[k]; m < boff[k + 1]; ++m) {
                    if (ids[m] != JG_NULL_ELEM) {
                        const std::string& e = h1.sets[k].names[ids[m]];
                        bbytes.insert(bbytes.end(), e.begin(), e.end());
                    }
                    bnoff.push_back(bbytes.size());
                }
            return ms_since(t0);
        };
        std::vector<double> a, b1, b2;
        for (int r = 0; r < warm + reps; ++r) {
            const double x = base(), y = by_name(), z = base();
            noff.resize(off[keys] + 1);
            require(off == boff && noff == bnoff && bytes == bbytes, "(c) LookupAll");
            if (r >= warm) a.push_back(y), b1.push_back(x), b2.push_back(z);
        }
        report("(c) LookupAll of every set", a, b1, b2);
        std::printf("    %llu members, %llu name bytes\n", (unsigned long long)off[keys], (unsigned long long)bytes.size());
    }
    jg_orset_destroy(sn), jg_orset_destroy(t1), jg_orset_destroy(t2);
    jg_close(ctx);
    return 0;
}
