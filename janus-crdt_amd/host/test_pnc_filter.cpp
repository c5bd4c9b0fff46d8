// test_pnc_filter.cpp — csrc/pnc_filter.hpp on the CPU (no device code): the per-cell arithmetic of the dense merge's
// 32-bit shadow over every ordered pair of edge values.  Prints one "ok <check>" line per check and "PASS" at the
// end; exits 1 at the first failure.  tests/test_pnc_filter.py runs it, plain and under the address and
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

long long ref_clamp(long long v) { return std::min<long long>(std::max<long long>(v, INT32_MIN), INT32_MAX); }

}  // namespace

int main() {
    using namespace jg::filt;
    long long a_ = 0, b_ = 0;
    for (long long v : kEdges) {
        a_ = v;
        CHECK((long long)clamp32(v) == ref_clamp(v));
        CHECK(known(clamp32(v)) == (v > INT32_MIN && v < INT32_MAX));
        if (known(clamp32(v))) CHECK((long long)clamp32(v) == v);  // a known shadow is the cell
    }
    std::printf("ok clamp\n");

    for (long long a : kEdges)
        for (long long b : kEdges) {
            a_ = a, b_ = b;
            const int32_t s = clamp32(a);
            // the merge of the cell itself
            const Merged r = merge_cell(a, b);
            CHECK(r.m == std::max(a, b));
            CHECK(r.changed == (b > a));
            CHECK((long long)r.s == ref_clamp(std::max(a, b)));
            // A is asked for exactly at an undecidable escape: the shadow is a clamp value, b is not ABSENT, and the
            // shadow does not already bound the cell above b
            const bool escape = s == INT32_MIN || s == INT32_MAX;
            const bool decidable = b == INT64_MIN || (s == INT32_MAX && b < INT32_MAX);
            CHECK(needs_a(s, b) == (escape && !decidable));
            CHECK(may_change(s, b) == (escape ? !decidable : b > a));
            // what the filtered kernel computes: A read where asked, else the shadow standing in for the cell
            const bool read = needs_a(s, b);
            const Merged f = merge_cell(cell_of(s, read, a), b);
            CHECK(f.changed == r.changed);
            if (f.changed || read || !escape) {  // the values are stored, or could be (a known neighbour of a raised cell)
                CHECK(f.m == r.m);
                CHECK(f.s == r.s);
            }
            // an escape that was not read merges to "unchanged", and its shadow stays what it was
            if (escape && !read) CHECK(!f.changed && f.s == s);
        }
    std::printf("ok pairs\n");
    std::printf("PASS %d checks\n", g_checks);
    return 0;
}
