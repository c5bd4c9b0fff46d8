// pnc_wire.hpp — the PNCounterMsg wire form on the device: the Guid and replica-table types, the serial parser
// that holds a payload to the decode contract (oracle/json.hpp, System.Text.Json 6.0's defaults), pass A's record
// format, and the serial bodies of passes A, C and B built on the parser (scan_one / resolve_one / apply_one).
// For json.hip (json_wave.hpp's group parse accepts a subset of this parser's) and pnc_encode.hip (it writes this form).
#pragma once

#include <type_traits>

#include "jg_internal.hpp"
#include "wire_cursor.hpp"

namespace {  // internal to each file that includes this, like the kernels that use it

constexpr int kBlock = 256;
constexpr uint32_t kMaxJsonReplicas = jg::kMaxTableReplicas;  // per-vector duplicate masks are 4 x 64 bits

enum : uint32_t { kErrSyntax = 0, kErrFull = 1, kErrInternal = 2 };

struct Guid16 { unsigned long long lo, hi; };

using jgw::Cursor, jgw::hexv;  // byte cursor with a 16-byte aligned window (wire_cursor.hpp)

// 36-char "D" Guid (Guid.ToString() layout: b3b2b1b0-b5b4-b7b6-b8b9-b10..b15) + the closing quote.
__device__ __forceinline__ bool read_guid(Cursor& c, Guid16& g) {
    unsigned long long lo = 0, hi = 0;
    // groups: a (8 hex) -> lo[0:32), b (4) -> lo[32:48), c (4) -> lo[48:64), then 8 bytes of hi in text order
    uint32_t v = 0;
    for (int i = 0; i < 8; ++i) { const int h = hexv(c.get()); if (h < 0) return false; v = v << 4 | (uint32_t)h; }
    lo = v;
    if (c.get() != '-') return false;
    v = 0;
    for (int i = 0; i < 4; ++i) { const int h = hexv(c.get()); if (h < 0) return false; v = v << 4 | (uint32_t)h; }
    lo |= (unsigned long long)v << 32;
    if (c.get() != '-') return false;
    v = 0;
    for (int i = 0; i < 4; ++i) { const int h = hexv(c.get()); if (h < 0) return false; v = v << 4 | (uint32_t)h; }
    lo |= (unsigned long long)v << 48;
    if (c.get() != '-') return false;
    for (int b = 0; b < 8; ++b) {
        if (b == 2 && c.get() != '-') return false;
        const int h = hexv(c.get()), l = hexv(c.get());
        if (h < 0 || l < 0) return false;
        hi |= (unsigned long long)(h << 4 | l) << (8 * b);
    }
    if (c.get() != '"') return false;
    g.lo = lo;
    g.hi = hi;
    return true;
}

// -?(0|[1-9][0-9]*) within the width (Utf8JsonReader.GetInt32 / GetInt64).
template <int EB>
__device__ __forceinline__ bool read_int(Cursor& c, long long& out) {
    c.ws();
    bool neg = false;
    int ch = c.peek();
    if (ch == '-') { neg = true; ++c.p; ch = c.peek(); }
    if (ch < '0' || ch > '9') return false;
    unsigned long long mag = 0;
    if (ch == '0') {
        ++c.p;
        ch = c.peek();
        if (ch >= '0' && ch <= '9') return false;  // leading zero
    } else {
        while (ch >= '0' && ch <= '9') {
            const unsigned d = (unsigned)(ch - '0');
            if (mag > (~0ull - d) / 10) return false;
            mag = mag * 10 + d;
            ++c.p;
            ch = c.peek();
        }
    }
    const unsigned long long lim = EB == 4 ? (neg ? 0x80000000ull : 0x7FFFFFFFull) : (neg ? 0x8000000000000000ull : 0x7FFFFFFFFFFFFFFFull);
    if (mag > lim) return false;
    out = neg ? (long long)(0ull - mag) : (long long)mag;
    return true;
}

// ---- the decode contract (oracle/json.hpp, System.Text.Json 6.0's defaults) ------------------------------------
// Property names are matched after unescaping; a member the type does not have is skipped (jgw::skip_value); a
// member given twice takes its last occurrence; a Guid key repeated inside one vector keeps its first place and
// takes its last value (Dictionary's indexer).  The compact form System.Text.Json writes — every state a reference
// node emits — is proven by the group parse (json_wave.hpp); the serial parser below runs only on the rest.

struct PncPropSink {  // "pVector" -> 0, "nVector" -> 1, anything else -> 2 (case-sensitive, unescaped)
    uint32_t len = 0, mask = 3;
    __device__ void esc() {}
    __device__ void put(int b) {
        const char* rest = "Vector";
        if (len == 0) mask &= (b == 'p' ? 1u : 0u) | (b == 'n' ? 2u : 0u);
        else if (len > 6 || rest[len - 1] != (char)b) mask = 0;
        ++len;
    }
    __device__ int which() const { return len == 7 && mask ? (mask & 1 ? 0 : 1) : 2; }
};

// A property name (after its opening quote has been found): 0 / 1 / 2 as PncPropSink, -1 if not a string.
__device__ __forceinline__ int read_prop(Cursor& c) {
    if (!c.expect('"')) return -1;
    PncPropSink ps;
    if (!jgw::read_string(c, ps)) return -1;
    return ps.which();
}

// A Guid key after its opening quote: the raw 36-character form, or (escapes) the unescaped string's.
__device__ __forceinline__ bool read_key(Cursor& c, Guid16& g) {
    Cursor t = c;
    if (read_guid(t, g)) {
        c = t;
        return true;
    }
    jgw::GuidSink gs;
    if (!jgw::read_string(c, gs) || !gs.ok()) return false;
    g.lo = gs.lo();
    g.hi = gs.hi;
    return true;
}

__device__ __forceinline__ bool same_guid(const Guid16& a, const Guid16& b) { return a.lo == b.lo && a.hi == b.hi; }

// Per vector, over the whole message: occurrences of the member, whether the last one is `null`, and whether the
// last one may repeat a key (a 128-bit filter of its keys: no shared bit = no repeat, so the common state skips the
// repeat scans).
struct VecInfo {
    uint32_t occ = 0;
    bool null_last = false, maybe_dup = false;
};

// The whole payload checked (every occurrence of every member, skipped ones included): true iff System.Text.Json
// decodes it and both vectors end non-null (else Merge would throw).  No visits.
template <int EB>
__device__ bool validate_pnc(Cursor& c, VecInfo (&vi)[2]) {
    if (!c.expect('{')) return false;
    c.ws();
    if (c.peek() == '}') return false;  // {}: both vectors missing
    for (;;) {
        const int which = read_prop(c);
        if (which < 0 || !c.expect(':')) return false;
        if (which == 2) {
            if (!jgw::skip_value(c, 1)) return false;
        } else {
            VecInfo& v = vi[which];
            ++v.occ;
            v.maybe_dup = false;
            c.ws();
            v.null_last = c.peek() == 'n';
            if (v.null_last) {
                if (!jgw::take_literal(c, "null")) return false;
            } else {
                if (!c.expect('{')) return false;
                unsigned long long f0 = 0, f1 = 0;
                c.ws();
                if (c.peek() == '}') {
                    ++c.p;
                } else {
                    for (;;) {
                        Guid16 g;
                        long long x;
                        if (!c.expect('"') || !read_key(c, g) || !c.expect(':') || !read_int<EB>(c, x)) return false;
                        const uint32_t h = (uint32_t)((g.lo ^ g.hi) * 0x9E3779B97F4A7C15ull >> 57);  // 7 bits
                        const unsigned long long b = 1ull << (h & 63);
                        const bool hit = (h & 64) ? (f1 & b) != 0 : (f0 & b) != 0;
                        v.maybe_dup |= hit;
                        if (h & 64) f1 |= b;
                        else f0 |= b;
                        c.ws();
                        const int ch = c.get();
                        if (ch == '}') break;
                        if (ch != ',') return false;
                    }
                }
            }
        }
        c.ws();
        const int ch = c.get();
        if (ch == '}') break;
        if (ch != ',') return false;
    }
    c.ws();
    return c.p == c.end && vi[0].occ && vi[1].occ && !vi[0].null_last && !vi[1].null_last;
}

// Parse one PNCounterMsg: vis.entry(which, pos, guid, value) for every entry of the decoded message (the last
// occurrence of each vector; a repeated key once, at its first place, with its last value; pos = its place among
// the vector's distinct keys), returning false to abort.  `only` = -1 visits both vectors, 0 / 1 only pVector /
// nVector; begin_vector(which) opens each visited occurrence either way.  The payload is validated whole first
// (validate_pnc), so a message is visited only if System.Text.Json decodes it.
template <int EB, class V>
__device__ bool parse_pnc(Cursor& c, V& vis, int only = -1) {
    VecInfo vi[2];
    {
        Cursor t = c;
        if (!validate_pnc<EB>(t, vi)) {
            c = t;
            return false;
        }
    }
    uint32_t occ[2] = {0, 0};
    (void)c.expect('{');
    for (;;) {
        const int which = read_prop(c);
        (void)c.expect(':');
        if (which == 2 || ++occ[which] < vi[which].occ) {
            (void)jgw::skip_value(c, 1);  // validated: a skipped member, or an occurrence a later one replaces
        } else {
            vis.begin_vector(which);
            (void)c.expect('{');
            c.ws();
            if (c.peek() == '}') {
                ++c.p;
            } else {
                const Cursor vstart = c;
                const bool dups = vi[which].maybe_dup;
                uint32_t pos = 0;
                for (;;) {
                    c.ws();
                    const uint64_t at = c.p;
                    Guid16 g;
                    long long v;
                    (void)c.expect('"');
                    (void)read_key(c, g);
                    (void)c.expect(':');
                    (void)read_int<EB>(c, v);
                    bool first = true;
                    if (dups) {  // a key met earlier in this vector was visited there; else its LAST value counts
                        Cursor t = vstart;
                        for (;;) {
                            t.ws();
                            if (t.p >= at) break;
                            Guid16 h;
                            long long y;
                            (void)t.expect('"');
                            (void)read_key(t, h);
                            (void)t.expect(':');
                            (void)read_int<EB>(t, y);
                            if (same_guid(h, g)) {
                                first = false;
                                break;
                            }
                            (void)t.expect(',');
                        }
                        if (first) {
                            Cursor t2 = c;
                            for (;;) {
                                t2.ws();
                                if (t2.get() != ',') break;
                                Guid16 h;
                                long long y;
                                (void)t2.expect('"');
                                (void)read_key(t2, h);
                                (void)t2.expect(':');
                                (void)read_int<EB>(t2, y);
                                if (same_guid(h, g)) v = y;
                            }
                        }
                    }
                    if (first) {
                        if ((only < 0 || only == which) && !vis.entry(which, pos, g, v)) return false;
                        ++pos;
                    }
                    c.ws();
                    if (c.get() == '}') break;
                }
            }
        }
        c.ws();
        if (c.get() == '}') break;
    }
    c.ws();
    return true;
}

// ---- replica table helpers -------------------------------------------------------------------------
struct Table {
    Guid16* cols;   // [n_keys x R]
    uint32_t* ncols;
    uint32_t R;
};

__device__ __forceinline__ uint32_t find_col(const Guid16* row, uint32_t n, const Guid16& g, uint32_t hint) {
    if (hint < n) {
        const Guid16 h = row[hint];
        if (h.lo == g.lo && h.hi == g.hi) return hint;
    }
    for (uint32_t j = 0; j < n; ++j) {
        const Guid16 h = row[j];
        if (h.lo == g.lo && h.hi == g.hi) return j;
    }
    return UINT32_MAX;
}

// 256-bit column mask without dynamic register indexing (no scratch spills).
struct Mask256 {
    unsigned long long w0 = 0, w1 = 0, w2 = 0, w3 = 0;
    __device__ void clear() { w0 = w1 = w2 = w3 = 0; }
    __device__ bool test_set(uint32_t c) {  // returns the old bit (no address taken: stays in registers)
        const unsigned long long b = 1ull << (c & 63);
        bool old;
        switch (c >> 6) {
            case 0: old = (w0 & b) != 0; w0 |= b; break;
            case 1: old = (w1 & b) != 0; w1 |= b; break;
            case 2: old = (w2 & b) != 0; w2 |= b; break;
            default: old = (w3 & b) != 0; w3 |= b; break;
        }
        return old;
    }
};

// Pass A visitor: unknown Guids mark the message deferred (parse_pnc visits a repeated key once).
struct ScanVis {
    const Guid16* row;
    uint32_t n;
    bool miss = false;
    __device__ void begin_vector(int) {}
    __device__ bool entry(int, uint32_t pos, const Guid16& g, long long) {
        if (find_col(row, n, g, pos) == UINT32_MAX) miss = true;
        return true;
    }
};

// Pass A's per-message output (json_wave.hpp writes it for the payloads it proves compact): a u16
// entry count (kReparse: pass B parses the message again), a u16 code per entry (column | vector << 15),
// then the entries' values at +32.  Entries in token order; at most kEmitMax.
constexpr uint32_t kEmitMax = 14;
constexpr uint16_t kReparse = 0xFFFF;
constexpr uint32_t kNeedsCols = 0x4000;  // count flag: a deferred record whose columns pass C resolves
constexpr uint32_t kVoidCol = 0x7FFF;    // entry code column of a voided entry (a key its vector repeats later)
constexpr uint32_t kApplied = 0x2000;    // count flag: pass A applied the message itself (fused); low bits = the
                                         // entries it raised, recorded as (column code, old value) for the undo
__host__ __device__ constexpr uint64_t emit_stride(uint32_t eb) { return 32 + kEmitMax * eb; }

// deferred[m] (pass A): row << 32 | m for a message naming a replica its row has not seen, else this.
constexpr unsigned long long kNotDeferred = ~0ull;

// Serial pass-A body for one message (one lane): the definitive parse.  A message it accepts is marked
// deferred (a replica its row has not seen) or, given a `slow` list, appended to it (pass B parses it
// again); k_scan_slow passes none: its messages are on the list already.
template <int EB>
__device__ void scan_one(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off, const uint32_t* __restrict__ rows, uint64_t m,
                         const Table& t, unsigned long long* __restrict__ status, unsigned long long* __restrict__ deferred,
                         uint8_t* __restrict__ emit, unsigned long long* __restrict__ slow) {
    const uint32_t row = rows[m];
    if (row == jg::kSkipIdx) {  // another kind's message in a node wave (csrc/node.hip): no entries
        *reinterpret_cast<uint16_t*>(emit + m * emit_stride(EB)) = 0;
        deferred[m] = kNotDeferred;
        return;
    }
    *reinterpret_cast<uint16_t*>(emit + m * emit_stride(EB)) = kReparse;
    Cursor c(bytes, off[m], off[m + 1]);
    ScanVis vis{t.cols + (uint64_t)row * t.R, t.ncols[row]};
    if (!parse_pnc<EB>(c, vis)) {
        atomicMin(status, (unsigned long long)m << 2 | kErrSyntax);
        return;
    }
    deferred[m] = vis.miss ? (unsigned long long)row << 32 | m : kNotDeferred;  // counted by select_deferred
    if (vis.miss) status[1] = 1;  // any deferral: the guarded tail of finish_wave stands down
    if (!vis.miss && slow) {
        const unsigned long long at = atomicAdd(status + 3, 1ull);
        slow[at] = m;
    }
}

// Pass C visitor: exclusive owner of the row; appends new Guids.  Merge visits every pVector entry
// before any nVector entry (PNCounters.cs:133-143): one parse covers both when pVector comes first in
// the text (every Encode'd state); an nVector ahead of its pVector is skipped and visited by a second
// parse (`only` = 1) once the pVector is in.
struct ResolveVis {
    Guid16* row;
    uint32_t* ncol;
    uint32_t R;
    uint32_t err = UINT32_MAX;
    bool p_seen = false, n_skipped = false;
    __device__ void begin_vector(int which) {
        if (which == 0) p_seen = true;
    }
    __device__ bool entry(int which, uint32_t pos, const Guid16& g, long long) {
        if (which == 1 && !p_seen) { n_skipped = true; return true; }
        uint32_t c = find_col(row, *ncol, g, pos);
        if (c == UINT32_MAX) {
            if (*ncol >= R) { err = kErrFull; return false; }
            c = (*ncol)++;
            row[c] = g;
        }
        return true;
    }
};

// One message of a row's walk (serial): new Guids appended to the row; returns an error code or UINT32_MAX.
template <int EB>
__device__ uint32_t resolve_msg(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off, uint64_t m, Guid16* row, uint32_t* ncol,
                                uint32_t R) {
    ResolveVis vis{row, ncol, R};
    Cursor c(bytes, off[m], off[m + 1]);
    bool ok = parse_pnc<EB>(c, vis);
    if (ok && vis.n_skipped) {
        Cursor c2(bytes, off[m], off[m + 1]);
        ok = parse_pnc<EB>(c2, vis, 1);
    }
    return ok ? UINT32_MAX : vis.err == UINT32_MAX ? kErrInternal : vis.err;
}

// Serial pass C for sorted deferred entry i: a segment head (first entry of a row) walks its row's
// messages in commit order.  saved[i] = the head's ncols before the walk (for roll-back).
template <int EB>
__device__ void resolve_one(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off, const unsigned long long* __restrict__ keys,
                            uint64_t nd, uint64_t i, const Table& t, uint32_t* __restrict__ saved, unsigned long long* __restrict__ status) {
    const uint32_t row = (uint32_t)(keys[i] >> 32);
    if (i > 0 && (uint32_t)(keys[i - 1] >> 32) == row) return;
    uint32_t* ncol = t.ncols + row;
    saved[i] = *ncol;
    for (uint64_t j = i; j < nd && (uint32_t)(keys[j] >> 32) == row; ++j) {
        const uint64_t m = (uint32_t)keys[j];
        const uint32_t err = resolve_msg<EB>(bytes, off, m, t.cols + (uint64_t)row * t.R, ncol, t.R);
        if (err != UINT32_MAX) {
            atomicMin(status + 2, (unsigned long long)m << 2 | err);
            return;
        }
    }
}

// Pass B visitor: max into the cells.
template <int EB>
struct ApplyVis {
    using T = typename std::conditional<EB == 4, int, long long>::type;
    T* P;
    T* N;
    const Guid16* row;
    uint32_t n;
    bool bad = false;
    __device__ void begin_vector(int) {}
    __device__ bool entry(int which, uint32_t pos, const Guid16& g, long long v) {
        const uint32_t c = find_col(row, n, g, pos);
        if (c == UINT32_MAX) { bad = true; return false; }
        atomicMax((which ? N : P) + c, (T)v);
        return true;
    }
};

template <int EB>
__device__ void apply_one(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off, const uint32_t* __restrict__ rows, uint64_t m,
                          const Table& t, void* P, void* N, unsigned long long* __restrict__ status) {
    using T = typename ApplyVis<EB>::T;
    const uint32_t row = rows[m];
    const uint64_t base = (uint64_t)row * t.R;
    Cursor c(bytes, off[m], off[m + 1]);
    ApplyVis<EB> vis{static_cast<T*>(P) + base, static_cast<T*>(N) + base, t.cols + base, t.ncols[row]};
    if (!parse_pnc<EB>(c, vis)) atomicMin(status + 2, (unsigned long long)m << 2 | kErrInternal);
}

}  // namespace
