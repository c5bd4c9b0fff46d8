// pnc_filter.hpp — the per-cell arithmetic of the dense PN-Counter merge's 32-bit shadow (HIP-free: the filtered
// kernel and the build launch in pnc_dense_kernels.hpp and host/test_pnc_filter.cpp share this one definition), and
// of the narrow form of a received cell (fits / narrow / widen: pnc_dense_kernels.hpp's batch kernels, host/test_pnc_narrow.cpp).
//
// The shadow of an int64 cell a is s = clamp32(a).  Strictly inside the int32 range the shadow IS the cell
// (a == (int64)s), so a merge needs no read of a; at the two clamp values ("escapes") it only bounds it:
// s == INT32_MAX means a >= INT32_MAX, s == INT32_MIN means a <= INT32_MIN.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JG_FILT_HD __host__ __device__ __forceinline__
#else
#define JG_FILT_HD inline
#endif

namespace jg {
namespace filt {

constexpr int32_t kLo = INT32_MIN, kHi = INT32_MAX;

JG_FILT_HD int32_t clamp32(long long v) { return v < (long long)kLo ? kLo : v > (long long)kHi ? kHi : (int32_t)v; }

// The narrow form of a received int64 cell b (a dense identity batch held as 4-byte codes, jg_rows): b fits if it is
// ABSENT (INT64_MIN) or INT32_MIN < b <= INT32_MAX; its code is INT32_MIN for ABSENT and (int32)b otherwise, so a real
// value of exactly INT32_MIN does not fit (that code is taken).  widen(narrow(b)) == b for every fitting b.
JG_FILT_HD bool fits(long long b) { return b == INT64_MIN || (b > (long long)kLo && b <= (long long)kHi); }
JG_FILT_HD int32_t narrow(long long b) { return b == INT64_MIN ? kLo : (int32_t)b; }
JG_FILT_HD long long widen(int32_t c) { return c == kLo ? INT64_MIN : (long long)c; }

// The shadow value determines the cell.
JG_FILT_HD bool known(int32_t s) { return s != kLo && s != kHi; }

// The merge of a cell whose shadow is s with a received b needs the cell itself: an escape whose outcome the
// shadow does not decide.  Decidable without it: b is ABSENT (INT64_MIN: nothing is below it), or the cell is at or
// above INT32_MAX and b is below INT32_MAX (b < a).  A known cell never asks.
JG_FILT_HD bool needs_a(int32_t s, long long b) {
    if (known(s)) return false;
    if (b == INT64_MIN) return false;
    if (s == kHi && b < (long long)kHi) return false;
    return true;
}

// The cell may change: what the filtered kernel can say before any read of A (exact for known cells, "has to
// look" for undecidable escapes).
JG_FILT_HD bool may_change(int32_t s, long long b) { return known(s) ? b > (long long)s : needs_a(s, b); }

struct Merged {
    long long m;   // max(a, b): the cell after the merge
    bool changed;  // m != a: its line of A (and of the shadow) has to be written
    int32_t s;     // the cell's new shadow
};

JG_FILT_HD Merged merge_cell(long long a, long long b) {
    const long long m = a > b ? a : b;
    return Merged{m, m != a, clamp32(m)};
}

// The cell as the filtered merge sees it: the shadow sign-extended, or `a_loaded` where A was read.  Where
// !needs_a(s, b) and A was not read, an escape cell stands in as its clamp value, which merges to "unchanged"
// (see needs_a), and its line is then not written unless another cell of the line forced the read of A.
JG_FILT_HD long long cell_of(int32_t s, bool a_read, long long a_loaded) { return a_read ? a_loaded : (long long)s; }

}  // namespace filt
}  // namespace jg
