// test_orset_walk.cpp — csrc/orset_walk.hpp (the index arithmetic of the OR-Set record walk on the device) on the CPU:
// no HIP, no library.  Random single-key scripts are walked sequentially over explicit tag sets and again through the
// header's functions over exclusive prefix sums and scanned marks, as the kernels do; the segment search is held to a
// linear one.  Built twice (Makefile): plain, and under the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "orset_walk.hpp"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t m) {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 33) % m);
}

int fails = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                                 \
        }                                                            \
    } while (0)

void test_last_le() {
    for (int round = 0; round < 2000; ++round) {
        const uint64_t n = 1 + rnd(40);
        std::vector<unsigned long long> off(n + 1, 0);
        for (uint64_t i = 0; i < n; ++i) off[i + 1] = off[i] + (rnd(3) ? 0 : rnd(5));
        for (unsigned long long j = 0; j < off[n]; ++j) {
            uint64_t want = 0;
            for (uint64_t p = 0; p < n; ++p)
                if (off[p] <= j) want = p;
            const uint64_t got = jgw::last_le(off.data(), n, j);
            CHECK(got == want);
            CHECK(off[got] <= j && j < off[got + 1]);  // the owner holds the item
        }
    }
}

// One segment (one key, one epoch) starting at position `seg` of a longer array of positions.
void test_segment() {
    for (int round = 0; round < 20000; ++round) {
        const uint32_t lead = rnd(4), len = 1 + rnd(14), n = lead + len + rnd(3);
        const uint32_t elem = rnd(2) ? jgw::kNullElem : 7;
        std::set<uint32_t> A0, R0;
        for (uint32_t t = 0; t < 6; ++t) {
            if (rnd(4) == 0) A0.insert(t);
            if (rnd(4) == 0) R0.insert(t);
        }
        jgw::Base b{A0.size(), R0.size(), 0, 0};
        for (uint32_t t : R0) b.m0 += !A0.count(t);
        for (uint32_t t : A0) b.u0 += !R0.count(t);
        std::vector<uint8_t> op(n, 0);
        std::vector<uint32_t> tag(n, 0), is(n, 0), fl(n, 0), ua(n, 0), marks(n, 0), revs(n, 0);
        std::set<uint32_t> seen;
        for (uint32_t p = 0; p < n; ++p) {
            const bool in = p >= lead && p < lead + len;
            op[p] = in ? 1 + rnd(3) : 1 + rnd(2);  // 1 Add, 2 Remove, 3 read (inside); other segments around it
            if (op[p] == 3) op[p] = 4;
            tag[p] = rnd(6);
            if (in && op[p] == 1) {
                is[p] = !A0.count(tag[p]) && seen.insert(tag[p]).second;
                fl[p] = is[p] && R0.count(tag[p]);
                ua[p] = is[p] && !fl[p];
            }
            marks[p] = jgw::mark(p, p == lead || p == lead + len || p == 0, op[p] == 2);
            revs[jgw::rev_slot(n, p)] = jgw::rev_mark(n, p, op[p] == 2);
        }
        std::vector<uint32_t> isx(n, 0), flx(n, 0), uax(n, 0);
        for (uint32_t p = 1; p < n; ++p) {
            isx[p] = isx[p - 1] + is[p - 1], flx[p] = flx[p - 1] + fl[p - 1], uax[p] = uax[p - 1] + ua[p - 1];
            marks[p] = marks[p] > marks[p - 1] ? marks[p] : marks[p - 1];
            revs[p] = revs[p] > revs[p - 1] ? revs[p] : revs[p - 1];
        }
        // the sequential walk of the segment
        std::set<uint32_t> add = A0, rem = R0;
        for (uint32_t p = lead; p < lead + len; ++p) {
            const uint32_t q = jgw::prev_remove(marks.data(), p, lead);
            uint32_t want_q = jgw::kNone;
            for (uint32_t x = lead; x < p; ++x)
                if (op[x] == 2) want_q = x;
            CHECK(q == want_q);
            uint32_t want_r = jgw::kNone;
            for (uint32_t x = n; x-- > p;)
                if (op[x] == 2) want_r = x;
            CHECK(jgw::next_remove(revs.data(), n, p) == want_r);
            const bool has = q != jgw::kNone;
            const jgw::State st = jgw::state_at(b, isx[p] - isx[lead], flx[p] - flx[lead], uax[p] - uax[lead], has, has ? uax[q] - uax[lead] : 0);
            uint64_t m = 0, u = 0;
            for (uint32_t t : rem) m += !add.count(t);
            for (uint32_t t : add) u += !rem.count(t);
            CHECK(st.nA == add.size() && st.nR == rem.size() && st.m == m && st.u == u);
            const bool differ = add != rem;
            CHECK(jgw::present(elem, st) == (elem == jgw::kNullElem ? differ : !add.empty() && (rem.empty() || differ)));
            if (op[p] == 1) {
                if (ua[p]) CHECK(jgw::uadd_slot(b, uax[p] - uax[lead], has, has ? uax[q] - uax[lead] : 0) == u);  // appended after the u pending ones
                add.insert(tag[p]);
            } else if (op[p] == 2) {
                for (uint32_t t : add) rem.insert(t);
            }
        }
    }
}

}  // namespace

int main() {
    test_last_le();
    test_segment();
    if (fails) return 1;
    std::printf("ok\n");
    return 0;
}
