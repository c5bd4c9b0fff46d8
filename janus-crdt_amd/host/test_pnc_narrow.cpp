// test_pnc_narrow.cpp — the narrow form of a received int64 cell (csrc/pnc_filter.hpp: fits, narrow, widen) on the CPU
// (no device code), and the merges a narrow batch takes part in, against plain int64 max: every ordered pair of the
// edge values test_pnc_filter.cpp uses plus the reserved code.  Prints one "ok <check>" line per check and "PASS" at the
// end; exits 1 at the first failure.  tests/test_pnc_narrow.py runs it, plain and under the address and
// undefined-behaviour sanitizers.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "pnc_filter.hpp"

namespace {

int g_checks = 0;
#define CHECK(cond)                                                                                       \
    do {                                                                                                  \
        if (!(cond)) {                                                                                    \
            std::printf("FAIL %s:%d: %s (a = %lld, b = %lld)\n", __FILE__, __LINE__, #cond, a_, b_);      \
            std::exit(1);                                                                                 \
        }                                                                                                 \
        ++g_checks;                                                                                       \
    } while (0)

const long long kEdges[] = {INT64_MIN, (long long)INT32_MIN - 1, INT32_MIN, (long long)INT32_MIN + 1, -1, 0, 1, (long long)INT32_MAX - 1,
                            INT32_MAX, 1ll << 31, 1ll << 40, INT64_MAX};

// the issue's definition, restated without the header's helpers
bool ref_fits(long long b) { return b == INT64_MIN || (b >= -2147483647ll && b <= 2147483647ll); }

}  // namespace

int main() {
    using namespace jg::filt;
    long long a_ = 0, b_ = 0;

    // fits: ABSENT and (INT32_MIN, INT32_MAX]; a real INT32_MIN does not (its code is ABSENT's)
    for (long long b : kEdges) {
        b_ = b;
        CHECK(fits(b) == ref_fits(b));
    }
    b_ = INT32_MIN;
    CHECK(!fits(INT32_MIN));
    CHECK(fits(INT64_MIN) && narrow(INT64_MIN) == INT32_MIN);
    CHECK(fits(INT32_MAX) && narrow(INT32_MAX) == INT32_MAX);
    CHECK(!fits((long long)INT32_MAX + 1) && !fits((long long)INT32_MIN - 1) && !fits(INT64_MAX));
    std::printf("ok fits\n");

    // round trips: cell -> code -> cell over the fitting edges, code -> cell -> code over the codes' edges
    for (long long b : kEdges) {
        b_ = b;
        if (!fits(b)) continue;
        CHECK(widen(narrow(b)) == b);
        CHECK((narrow(b) == INT32_MIN) == (b == INT64_MIN));
    }
    const int32_t kCodes[] = {INT32_MIN, INT32_MIN + 1, -1, 0, 1, INT32_MAX - 1, INT32_MAX};
    for (int32_t c : kCodes) {
        b_ = c;
        CHECK(fits(widen(c)));
        CHECK(narrow(widen(c)) == c);
        CHECK(widen(c) == (c == INT32_MIN ? INT64_MIN : (long long)c));
    }
    std::printf("ok roundtrip\n");

    // the merge of a store cell a with a fitting received cell that arrives as its code: the unfiltered merge, and the
    // filtered merge by a's shadow (the kernels widen the code, then run the wide batch's arithmetic)
    for (long long a : kEdges)
        for (long long b : kEdges) {
            a_ = a, b_ = b;
            if (!fits(b)) continue;
            const long long w = widen(narrow(b));
            const Merged r = merge_cell(a, w);
            CHECK(r.m == std::max(a, b));
            CHECK(r.changed == (b > a));
            CHECK(r.s == clamp32(std::max(a, b)));
            const int32_t s = clamp32(a);
            const bool read = needs_a(s, w);
            CHECK(may_change(s, w) == may_change(s, b) && read == needs_a(s, b));
            const Merged f = merge_cell(cell_of(s, read, a), w);
            CHECK(f.changed == r.changed);
            if (f.changed || read || known(s)) {
                CHECK(f.m == r.m);
                CHECK(f.s == r.s);
            }
            if (!known(s) && !read) CHECK(!f.changed && f.s == s);
            // an ABSENT code never changes a cell and never asks for it
            if (b == INT64_MIN) CHECK(!r.changed && !may_change(s, w));
        }
    std::printf("ok pairs\n");
    std::printf("PASS %d checks\n", g_checks);
    return 0;
}
