// host/bench_exec.cpp — a client stream with its "gp" reads in order among the writes, in one call (jg_node_exec_keys,
// csrc/update.hip), beside what the parent's entry points can do with the same commands:
//   (A) the floor: the reads hoisted into one jg_node_query_keys, then one jg_node_update_keys_ship over the writes.  A read
//       behind a write of its key gets the wrong answer this way, so only the writes' outputs are compared; it is the cost
//       of two calls over the same commands.  Run twice per repetition: the distance of its two medians is the A/A spread.
//   (B) the exact composition: the batch cut into maximal runs of reads / writes, one call per run, on the first 20,000
//       commands so that it finishes.  Everything is compared, the reads' values included.
// Shapes:
//   (1) PNCWorkload mix (PNCWorkload.cs:44-59): 100 PN-Counter keys x 4 int32 columns round-robin, 0.25 "i" / 0.25 "d" /
//       0.5 "gp", 250k commands
//   (2) ORSetWorkload mix (ORSetWorkload.cs:66-138): 10,000 sets filled as in bench_names, Adds of random 5-character names
//       and "gp" of a name the set was given earlier, half and half, a set cleared when it holds 50, 200k commands
// bench_update_ship's method: every way has stores of its own over one key space, every repetition gives all of them the
// same batch, outputs and stores are compared afterwards, outside the timed part.  Wall time of the calls a caller makes
// (the split of the batch into the parent's calls is prepared outside it); 2 warm-ups, median of 7, the ways alternating and
// taking turns at each place of a repetition;
// the same for (B).  Every way's output arrays are sized before its timed part.
// `--events`: one repetition per shape with JANUS_TRACE_UPDATE and JANUS_TRACE_QUERY set: the library reports its steps.
// usage: bench_exec [--events] [--shape 1|2] [--snap 1|2]
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
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

struct Strings {
    std::vector<uint64_t> off{0};
    std::string bytes;
    void push(const std::string& s) { bytes += s, off.push_back(bytes.size()); }
    std::string at(uint64_t i) const { return bytes.substr(off[i], off[i + 1] - off[i]); }
    uint64_t n() const { return off.size() - 1; }
    const uint8_t* data() const { return reinterpret_cast<const uint8_t*>(bytes.empty() ? "" : bytes.data()); }
};

struct Copy {
    jg_pnc* pnc = nullptr;
    jg_orset* ors = nullptr;
    jg_node* node = nullptr;
};
constexpr int kCopies = 5;  // 0: one call, 1 and 2: the floor, 3: one call on the short batch, 4: the exact composition
struct World {
    jg_ctx* ctx;
    jg_keyspace* ks = nullptr;
    Copy c[kCopies];
    void make(uint64_t pnc_keys, bool orset) {
        for (Copy& x : c) {
            if (pnc_keys) check(jg_pnc_create(ctx, pnc_keys, 4, 4, &x.pnc), "jg_pnc_create");
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
    void add_keys(const char* prefix, uint64_t n, uint8_t type) {
        Strings k;
        std::vector<jg_guid> g(n);
        std::vector<uint8_t> t(n, type);
        std::vector<uint32_t> idx(n);
        for (uint64_t i = 0; i < n; ++i) {
            k.push(prefix + std::to_string(i));
            g[i] = jg_guid{0x1000000 + i * 2 + type, 0xC0FFEE0000000000ull ^ (i * 0x9E3779B97F4A7C15ull)};
            idx[i] = (uint32_t)i;
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

struct Batch {  // commands in one order: reads (cmd 1) and writes (cmd 0)
    Strings keys, elems;
    std::vector<uint8_t> cmd, op, flag, snap;
    std::vector<int64_t> amount;
    std::vector<uint64_t> lo, hi;
    uint64_t n() const { return cmd.size(); }
    Batch part(uint64_t from, uint64_t to, int only = -1) const {  // commands [from, to), only those of one kind
        Batch b;
        for (uint64_t i = from; i < to; ++i) {
            if (only >= 0 && cmd[i] != only) continue;
            b.keys.push(keys.at(i)), b.elems.push(elems.at(i)), b.cmd.push_back(cmd[i]), b.op.push_back(op[i]), b.flag.push_back(flag[i]);
            b.snap.push_back(snap[i]), b.amount.push_back(amount[i]), b.lo.push_back(lo[i]), b.hi.push_back(hi[i]);
        }
        return b;
    }
};

struct Out {  // per command
    std::vector<uint8_t> status, result, sha, image;
    std::vector<int64_t> value;
    std::vector<uint64_t> off;
    uint64_t nb = 0;
    uint32_t rounds = 0;
    void reset(uint64_t n) { status.assign(n, 0), result.assign(n, 0), sha.assign(32 * n, 0), value.assign(n, 0), off.assign(n + 1, 0), rounds = 0; }
};

// keeps its buffer from one repetition to the next, as a caller does
void fetch(jg_node* node, uint64_t nb, std::vector<uint8_t>& arena) {
    if (nb <= arena.size()) return;
    arena.resize(nb + nb / 4);
    check(jg_node_shipped(node, &nb, arena.data(), arena.size()), "jg_node_shipped");
}

double one_call(World& w, Copy& c, const Batch& b, Out& o, std::vector<uint8_t>& arena) {
    const uint64_t n = b.n();
    o.reset(n);
    if (arena.empty()) arena.resize(16);
    const auto t0 = Clock::now();
    uint64_t nb = 0;
    check(jg_node_exec_keys(c.node, w.ks, n, b.keys.off.data(), b.keys.data(), b.cmd.data(), b.op.data(), b.flag.data(), b.amount.data(), b.elems.off.data(),
                            b.elems.data(), b.lo.data(), b.hi.data(), 0, b.snap.data(), o.status.data(), o.result.data(), o.value.data(), nullptr, nullptr,
                            nullptr, nullptr, o.off.data(), &nb, arena.data(), arena.size(), o.sha.data(), &o.rounds), "jg_node_exec_keys");
    fetch(c.node, nb, arena);
    const double ms = ms_since(t0);
    o.image.assign(arena.begin(), arena.begin() + nb);
    return ms;
}

// keep: the bytes are copied out of the arena inside the call's time (the next call of the way overwrites them)
void writes_call(World& w, Copy& c, const Batch& b, Out& o, std::vector<uint8_t>& arena, bool keep) {
    const uint64_t n = b.n();
    if (arena.empty()) arena.resize(16);
    uint64_t nb = 0;
    check(jg_node_update_keys_ship(c.node, w.ks, n, b.keys.off.data(), b.keys.data(), b.op.data(), b.flag.data(), b.amount.data(), b.elems.off.data(),
                                   b.elems.data(), b.lo.data(), b.hi.data(), 0, b.snap.data(), o.status.data(), o.result.data(), nullptr, nullptr, nullptr,
                                   nullptr, o.off.data(), &nb, arena.data(), arena.size(), o.sha.data(), &o.rounds), "jg_node_update_keys_ship");
    fetch(c.node, nb, arena);
    o.nb = nb;
    if (keep) o.image.assign(arena.begin(), arena.begin() + nb);
}

void reads_call(World& w, Copy& c, const Batch& b, Out& o, bool elems) {
    const uint64_t n = b.n();
    check(jg_node_query_keys(c.node, w.ks, n, b.keys.off.data(), b.keys.data(), elems ? b.elems.off.data() : nullptr, elems ? b.elems.data() : nullptr,
                             elems ? b.flag.data() : nullptr, o.value.data(), o.status.data(), nullptr, nullptr), "jg_node_query_keys");
}

// (A): two calls over the batch's reads and writes, split beforehand
double floor_way(World& w, Copy& c, const Batch& reads, const Batch& writes, bool elems, Out& ro, Out& wo, std::vector<uint8_t>& arena) {
    ro.reset(reads.n()), wo.reset(writes.n());
    if (arena.empty()) arena.resize(16);
    const auto t0 = Clock::now();
    if (reads.n()) reads_call(w, c, reads, ro, elems);
    if (writes.n()) writes_call(w, c, writes, wo, arena, false);
    const double ms = ms_since(t0);
    wo.image.assign(arena.begin(), arena.begin() + wo.nb);
    return ms;
}

// (B): one call per maximal run, prepared beforehand; the outputs gathered by command index outside the timed part
struct Run { Batch b; uint64_t from; Out o; };
double exact_way(World& w, Copy& c, std::vector<Run>& runs, bool elems, std::vector<uint8_t>& arena) {
    for (Run& r : runs) r.o.reset(r.b.n());
    if (arena.empty()) arena.resize(16);
    const auto t0 = Clock::now();
    for (Run& r : runs)
        if (r.b.cmd[0]) reads_call(w, c, r.b, r.o, elems);
        else writes_call(w, c, r.b, r.o, arena, true);
    return ms_since(t0);
}

void same_stores(World& w, int x, int y, uint64_t pnc_rows) {
    if (w.c[x].ors) {
        std::vector<jg_tagrec> a[2], r[2];
        const int cs[2] = {x, y};
        for (int k = 0; k < 2; ++k) {
            uint64_t na = 0, nr = 0;
            check(jg_orset_size(w.c[cs[k]].ors, &na, &nr), "jg_orset_size");
            a[k].resize(na), r[k].resize(nr);
            check(jg_orset_read(w.c[cs[k]].ors, a[k].data(), na, r[k].data(), nr), "jg_orset_read");
        }
        // (B) applies its writes call by call, so its ords differ from one call's: keys and tags are compared
        const auto same = [](const std::vector<jg_tagrec>& p, const std::vector<jg_tagrec>& q) {
            if (p.size() != q.size()) return false;
            for (size_t i = 0; i < p.size(); ++i)
                if (p[i].key != q[i].key || p[i].tag_lo != q[i].tag_lo || p[i].tag_hi != q[i].tag_hi) return false;
            return true;
        };
        require(same(a[0], a[1]) && same(r[0], r[1]), "the OR-Set stores agree");
    }
    if (w.c[x].pnc) {
        std::vector<int64_t> v[2];
        std::vector<uint8_t> o[2];
        const int cs[2] = {x, y};
        for (int k = 0; k < 2; ++k) {
            v[k].resize(pnc_rows), o[k].resize(pnc_rows);
            check(jg_pnc_values(w.c[cs[k]].pnc, nullptr, pnc_rows, v[k].data(), o[k].data()), "jg_pnc_values");
        }
        require(v[0] == v[1] && o[0] == o[1], "the PN-Counter stores agree");
    }
}

template <class Next> void run(const char* what, World& w, Next&& next, bool elems, uint64_t pnc_rows, bool events) {
    const int warm = events ? 1 : 2, reps = events ? 1 : 7;
    std::vector<double> t, a1, a2, by_place[3];
    std::vector<uint8_t> arena[kCopies];
    uint64_t n = 0, n_reads = 0, bytes = 0;
    uint32_t rounds = 0;
    for (int r = 0; r < warm + reps; ++r) {
        const Batch b = next(0);
        const Batch reads = b.part(0, b.n(), 1), writes = b.part(0, b.n(), 0);
        n = b.n(), n_reads = reads.n();
        Out o, ro1, wo1, ro2, wo2;
        // the three runs take turns at being first, second and third of a repetition: what a run's place costs it (the
        // first run of a repetition follows the host's batch generation, the others follow a run) is then spread over
        // the ways alike, and the medians by place are printed beside the medians by way
        double x = 0, y = 0, z = 0;
        for (int place = 0; place < 3; ++place) {
            const int way = (place + r) % 3;
            double& ms = way == 0 ? x : way == 1 ? y : z;
            if (way == 0) ms = floor_way(w, w.c[1], reads, writes, elems, ro1, wo1, arena[1]);
            else if (way == 1) ms = one_call(w, w.c[0], b, o, arena[0]);
            else ms = floor_way(w, w.c[2], reads, writes, elems, ro2, wo2, arena[2]);
            if (r >= warm) by_place[place].push_back(ms);
        }
        // the writes' outputs: status, result, bytes, hashes, rounds
        uint64_t k = 0;
        for (uint64_t i = 0; i < n; ++i) {
            if (b.cmd[i]) {
                require(o.off[i + 1] == o.off[i] && o.result[i] == 0 && o.status[i] == JG_Q_OK, "a read ships nothing and resolves");
                continue;
            }
            const uint64_t len = o.off[i + 1] - o.off[i];
            require(o.status[i] == wo1.status[k] && o.result[i] == wo1.result[k] && len == wo1.off[k + 1] - wo1.off[k] &&
                        !std::memcmp(o.image.data() + o.off[i], wo1.image.data() + wo1.off[k], len) &&
                        !std::memcmp(o.sha.data() + 32 * i, wo1.sha.data() + 32 * k, 32),
                    "one call ships for the writes what the floor's ship call ships");
            ++k;
        }
        require(o.rounds == wo1.rounds && wo1.image == wo2.image, "rounds, and the floor's two runs agree");
        same_stores(w, 0, 1, pnc_rows), same_stores(w, 0, 2, pnc_rows);
        bytes = o.image.size(), rounds = o.rounds;
        if (r >= warm) t.push_back(y), a1.push_back(x), a2.push_back(z);
        for (int c = 3; c <= 4; ++c) one_call(w, w.c[c], b, o, arena[c]);  // (B)'s two copies follow, untimed
    }
    const double m = median(t), m1 = median(a1), m2 = median(a2), base = std::min(m1, m2), spread = std::abs(m1 - m2);
    std::printf("%s: one call %.3f ms; (A) the floor, two calls %.3f / %.3f ms (A/A spread %.3f ms = %.1f%%); one call is %.2fx the floor: %s\n", what, m, m1,
                m2, spread, 100 * spread / base, m / base, m <= base + spread ? "within the bar" : "SLOWER than the floor");
    std::printf("    by place in the repetition, whichever way ran there: first %.3f ms, second %.3f ms, third %.3f ms\n", median(by_place[0]),
                median(by_place[1]), median(by_place[2]));
    std::printf("    %llu commands, %llu of them reads, %u rounds, %llu snapshot bytes = %.3f ms on the host link at 57 GB/s\n", (unsigned long long)n,
                (unsigned long long)n_reads, rounds, (unsigned long long)bytes, bytes / 57e9 * 1e3);
    std::fflush(stdout);
    if (events) return;

    // (B) on 20,000 commands: copies 3 (one call) and 4 (cut into runs) start from the same state as each other
    std::vector<double> tb, te;
    for (int r = 0; r < warm + reps; ++r) {
        const Batch b = next(20000);
        std::vector<Run> runs;
        for (uint64_t i = 0; i < b.n();) {
            uint64_t j = i;
            while (j < b.n() && b.cmd[j] == b.cmd[i]) ++j;
            runs.push_back(Run{b.part(i, j), i, Out{}});
            i = j;
        }
        Out o;
        const double y = one_call(w, w.c[3], b, o, arena[3]);
        const double x = exact_way(w, w.c[4], runs, elems, arena[4]);
        for (const Run& q : runs)
            for (uint64_t k = 0; k < q.b.n(); ++k) {
                const uint64_t i = q.from + k, len = o.off[i + 1] - o.off[i];
                require(o.status[i] == q.o.status[k] && o.value[i] == q.o.value[k], "status and value equal the exact composition's");
                if (b.cmd[i]) continue;
                require(o.result[i] == q.o.result[k] && len == q.o.off[k + 1] - q.o.off[k] &&
                            !std::memcmp(o.image.data() + o.off[i], q.o.image.data() + q.o.off[k], len) &&
                            !std::memcmp(o.sha.data() + 32 * i, q.o.sha.data() + 32 * k, 32),
                        "result, bytes and hash equal the exact composition's");
            }
        same_stores(w, 3, 4, pnc_rows);
        if (r >= warm) te.push_back(y), tb.push_back(x);
        n = runs.size();
    }
    std::printf("    (B) the exact composition on 20000 commands: one call %.3f ms; %llu alternating calls %.3f ms; one call is %.3fx: %s\n", median(te),
                (unsigned long long)n, median(tb), median(te) / median(tb), median(te) < median(tb) ? "faster" : "NOT faster");
    std::fflush(stdout);
}

}  // namespace

int main(int argc, char** argv) {
    bool events = false;
    int only = 0, snap_all = 1;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--events")) events = true;
        else if (!std::strcmp(argv[i], "--shape") && i + 1 < argc) only = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--snap") && i + 1 < argc) snap_all = std::atoi(argv[++i]);
    }
    if (events) setenv("JANUS_TRACE_UPDATE", "1", 1), setenv("JANUS_TRACE_QUERY", "1", 1);  // the library latches them at its first call
    std::mt19937_64 rng(2029);
    jg_ctx* ctx = nullptr;
    check(jg_open(0, &ctx), "jg_open");
    if (!only || only == 1) {
        World w{ctx};
        check(jg_keyspace_create(ctx, 1024, 1 << 16, &w.ks), "jg_keyspace_create");
        w.make(100, false);
        w.add_keys("key-", 100, 0);
        uint64_t at = 0;
        run("(1) PNCWorkload mix: 100 keys x 4 int32 columns round-robin, 0.25 i / 0.25 d / 0.5 gp", w, [&](uint64_t n) {
            Batch b;
            for (uint64_t i = 0; i < (n ? n : 250000); ++i, ++at) {
                const uint64_t draw = rng() % 4;  // 0, 1: "gp"; 2: "i"; 3: "d"
                b.keys.push("key-" + std::to_string(at % 100)), b.elems.push(""), b.cmd.push_back(draw < 2), b.op.push_back(draw == 3 ? 2 : 1);
                b.flag.push_back(draw < 2 ? 0 : 3), b.amount.push_back(1 + (int64_t)(rng() % 1000)), b.lo.push_back(0), b.hi.push_back(0);
                b.snap.push_back((uint8_t)snap_all);
            }
            return b;
        }, false, 100, events);
        w.destroy();
    }
    if (!only || only == 2) {
        const uint64_t sets = 10000, batch = 200000, fill_batches = 15;  // bench_names' resident store
        World w{ctx};
        check(jg_keyspace_create(ctx, sets + 256, sets * 64 + (1 << 14), &w.ks), "jg_keyspace_create");
        w.make(0, true);
        w.add_keys("set", sets, 1);
        std::vector<std::vector<std::string>> live(sets);  // the names each set was given since its last Clear
        const auto write_command = [&](uint64_t k, uint8_t& op, std::string& e) {
            e.clear();
            if (live[k].size() >= 50) {  // ORSetWorkload.cs:37-50
                live[k].clear(), op = 3;
                return;
            }
            for (int c = 0; c < 5; ++c) e.push_back(kChars[rng() % (sizeof kChars - 1)]);
            live[k].push_back(e), op = 1;
        };
        for (uint64_t f = 0; f < fill_batches; ++f) {
            std::vector<uint32_t> set;
            std::vector<uint8_t> op, is_null(batch, 0), res(batch);
            std::vector<uint64_t> lo, hi;
            Strings names;
            for (uint64_t i = 0; i < batch; ++i) {
                const uint64_t k = rng() % sets;
                uint8_t o;
                std::string e;
                write_command(k, o, e);
                set.push_back((uint32_t)k), op.push_back(o), names.push(e), lo.push_back(rng() | 1), hi.push_back(rng());
            }
            for (Copy& c : w.c)
                check(jg_orset_apply_ops_names(c.ors, batch, set.data(), op.data(), names.off.data(), names.data(), is_null.data(), lo.data(), hi.data(),
                                               res.data(), nullptr, nullptr, nullptr), "jg_orset_apply_ops_names");
        }
        run("(2) ORSetWorkload mix: 10,000 sets, Adds of 5-character names and gp of a name added earlier, half and half, Clear at 50", w, [&](uint64_t n) {
            Batch b;
            for (uint64_t i = 0; i < (n ? n : batch); ++i) {
                const uint64_t k = rng() % sets;
                b.keys.push("set" + std::to_string(k)), b.amount.push_back(0), b.snap.push_back((uint8_t)snap_all);
                if (rng() & 1) {  // "gp" of a name the set was given (a fresh one where it holds none)
                    std::string e = live[k].empty() ? std::string("none.") : live[k][rng() % live[k].size()];
                    b.elems.push(e), b.cmd.push_back(1), b.op.push_back(0), b.flag.push_back(1), b.lo.push_back(0), b.hi.push_back(0);
                    continue;
                }
                uint8_t o;
                std::string e;
                write_command(k, o, e);
                b.elems.push(e), b.cmd.push_back(0), b.op.push_back(o), b.flag.push_back(o == 3 ? 0 : 1), b.lo.push_back(rng() | 1), b.hi.push_back(rng());
            }
            return b;
        }, true, 0, events);
        w.destroy();
    }
    jg_close(ctx);
    return 0;
}
