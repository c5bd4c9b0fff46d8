// tpset_wire.hpp — the accepted wire form of a TPSetMsg (MergeSharp/MergeSharp/CRDTs/2P-Set.cs:49-60): the string
// sinks that name its members and hash its elements, the whitespace rule, and the serial parser that defines which
// messages apply and how far (oracle/json.hpp's contract).  Device-only; the parallel scanner (tpset_scan.hpp) proves
// a message flat against this parser, and tpset.hip runs it over every message the scanner could not prove.
#pragma once

#include "tpset_dict.hpp"
#include "wire_cursor.hpp"

namespace {  // internal to the file that includes this, like the kernels that use it

// ---- JSON string sinks ---------------------------------------------------------------------------
__constant__ char kMember[2][12] = {"addSet", "removeSet"};

struct NameSink {  // which TPSetMsg member a property name is, after unescaping (as System.Text.Json matches)
    uint32_t len = 0;
    bool ma = true, mr = true;
    __device__ void esc() {}
    __device__ void put(int b) {
        ma = ma && len < 6 && b == kMember[0][len];
        mr = mr && len < 9 && b == kMember[1][len];
        ++len;
    }
    __device__ int which() const { return ma && len == 6 ? 0 : mr && len == 9 ? 1 : -1; }
};

struct HashSink {  // the unescaped bytes into `out`, and their FNV-1a
    uint8_t* out;
    uint32_t n = 0;
    uint64_t h = jgt::kFnvBasis;
    __device__ void esc() {}
    __device__ void put(int b) {
        out[n++] = (uint8_t)b;
        h = (h ^ (uint64_t)(b & 0xFF)) * jgt::kFnvPrime;
    }
};

__device__ __forceinline__ bool is_ws(int c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }

// the first byte that is not JSON whitespace in [p, end), -1 if none
__device__ int next_token(const uint8_t* bytes, uint64_t p, uint64_t end) {
    for (; p < end; ++p)
        if (!is_ws(bytes[p])) return bytes[p];
    return -1;
}

// ---- the serial parser: the definition of the accepted wire form (oracle/json.hpp's contract) ------
// 0 = both members, 1 = nothing applies (malformed, or addSet missing / null), 2 = addSet only (removeSet missing /
// null).  pos[w] / cnt[w]: the byte after '[' and the element count of member w's LAST occurrence.
__device__ int parse_serial(const uint8_t* bytes, uint64_t beg, uint64_t end, uint64_t pos[2], uint32_t cnt[2]) {
    jgw::Cursor c(bytes, beg, end);
    bool seen[2] = {false, false}, null_last[2] = {false, false};
    if (!c.expect('{')) return 1;
    c.ws();
    if (c.peek() == '}') {
        ++c.p;
    } else {
        for (;;) {
            if (!c.expect('"')) return 1;
            NameSink ns;
            if (!jgw::read_string(c, ns)) return 1;
            if (!c.expect(':')) return 1;
            const int w = ns.which();
            if (w < 0) {
                if (!jgw::skip_value(c, 1)) return 1;
            } else {
                c.ws();
                seen[w] = true;
                if (c.peek() == 'n') {
                    if (!jgw::take_literal(c, "null")) return 1;
                    null_last[w] = true;
                } else {
                    if (!c.expect('[')) return 1;
                    null_last[w] = false;
                    pos[w] = c.p;
                    uint32_t k = 0;
                    c.ws();
                    if (c.peek() == ']') {
                        ++c.p;
                    } else {
                        for (;;) {
                            c.ws();
                            const int ch = c.peek();
                            if (ch == '"') {
                                ++c.p;
                                jgw::NullSink s;
                                if (!jgw::read_string(c, s)) return 1;
                            } else if (ch == 'n') {
                                if (!jgw::take_literal(c, "null")) return 1;
                            } else {
                                return 1;
                            }
                            ++k;
                            c.ws();
                            const int d = c.get();
                            if (d == ',') continue;
                            if (d == ']') break;
                            return 1;
                        }
                    }
                    cnt[w] = k;
                }
            }
            c.ws();
            const int d = c.get();
            if (d == ',') continue;
            if (d == '}') break;
            return 1;
        }
    }
    c.ws();
    if (c.p != end) return 1;
    if (!seen[0] || null_last[0]) return 1;
    if (!seen[1] || null_last[1]) return 2;
    return 0;
}

}  // namespace
