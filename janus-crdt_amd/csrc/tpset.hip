// tpset.hip — one TPSet<string?> resident on the device (MergeSharp/MergeSharp/CRDTs/2P-Set.cs): the replicated
// key-space set of BFT-CRDT/CRDTManagers/KeySpaceManager.cs:34,87.  DESIGN.md §Key-space set.
//
// Layout.  Nothing is ever removed from either HashSet, so a HashSet enumerates in first-insertion order and the
// ordinal of a string is its index in an append-only array: add[] and rem[] hold string ids in insertion order
// (kNullId = the C# null element), every distinct string lives once in the byte pool (soff / slen), sadd / srem give
// its ordinal in either array (kNone = not in it), and one open-addressing table maps the salted string hash to the
// string id (strings compared byte for byte on a hash match).
//
// Merge of a call's messages, every launch ordered on the context's stream (no workgroup waits on another):
//   scanner (mode 0)  k_tile_fn -> k_tile_carry -> k_mark -> scan -> k_emit -> k_strings -> k_walk
//   serial            k_serial (every message the scanner could not prove flat; all of them in mode 1)
//   candidates        scan of the per-array counts, k_place / k_serial_emit, k_cand_hash
//   insertion         k_cand_find (resident lookup, call-wide table, atomicMin of the candidate index per string)
//                     -> k_cand_win -> four scans -> k_commit_strings -> k_commit_entries
// The winner per distinct string is its first candidate in (message, addSet before removeSet, array position) order
// and winners are appended in that order, so ordinals equal the reference's insertion order.
#include <algorithm>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "launch.hpp"
#include "tpset_dict.hpp"
#include "wire_cursor.hpp"

using namespace jgt;  // the store / dictionary views and their probes (shared with query.hip)

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kTile = kBlock * 16;  // bytes of one scanner tile: 16 B per lane
constexpr uint32_t kNullId = 0xFFFFFFFEu;  // the null element's id in add[] / rem[]

using jg::blocks_for;

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
    uint64_t h = kFnvBasis;
    __device__ void esc() {}
    __device__ void put(int b) {
        out[n++] = (uint8_t)b;
        h = (h ^ (uint64_t)(b & 0xFF)) * kFnvPrime;
    }
};

__device__ __forceinline__ uint64_t umin(uint64_t a, uint64_t b) { return a < b ? a : b; }
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

// ---- the parallel scanner ------------------------------------------------------------------------
// State between two bytes: bit 0 = the next byte is escaped (an odd run of backslashes ends here), bit 1 = inside a
// string.  A span of bytes is a map over the four states, one byte per state; maps compose, so a block scan over the
// lanes' maps and one serial scan over the tiles' maps give every lane its state without a second look at the bytes
// before it.  The map of a message's first tile is made constant (its carry-in is state 0 whatever came before): the
// scan over tiles is segmented at message starts by the maps themselves, and a broken message cannot leak into the
// next one.
constexpr uint32_t kIdent = 0x03020100u;
__device__ __forceinline__ uint32_t fn_apply(uint32_t f, uint32_t s) { return (f >> (8 * s)) & 3; }
__device__ __forceinline__ uint32_t fn_then(uint32_t a, uint32_t b) {  // a, then b
    uint32_t r = 0;
#pragma unroll
    for (uint32_t s = 0; s < 4; ++s) r |= fn_apply(b, fn_apply(a, s)) << (8 * s);
    return r;
}

struct MsgScan {  // what k_mark gathers per message
    ull lbr_min, lbr_max, rbr_min, rbr_max;  // byte positions of '[' and ']' outside strings
    uint32_t n_lbrace, n_rbrace, n_lbr, n_rbr, n_colon;
    uint32_t notflat;
    uint32_t end_state;  // scanner state after the message's last byte
    uint32_t pad;
};

// the lane's 16 bytes of tile `tile`; bytes outside the message read as spaces
__device__ __forceinline__ void load_chunk(const uint8_t* bytes, uint64_t at, uint64_t lo, uint64_t hi, uint8_t (&b)[16]) {
    uint4 v = {0x20202020u, 0x20202020u, 0x20202020u, 0x20202020u};
    if (at < hi && at + 16 > lo) v = *reinterpret_cast<const uint4*>(bytes + at);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint64_t p = at + j;
        b[j] = p >= lo && p < hi ? (uint8_t)(w[j >> 2] >> (8 * (j & 3))) : (uint8_t)' ';
    }
}

__device__ __forceinline__ uint32_t chunk_fn(const uint8_t (&b)[16]) {
    uint32_t oe[2], qp[2];
#pragma unroll
    for (uint32_t e = 0; e < 2; ++e) {
        uint32_t esc = e, q = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (esc) esc = 0;
            else if (b[j] == '\\') esc = 1;
            else if (b[j] == '"') q ^= 1;
        }
        oe[e] = esc, qp[e] = q;
    }
    uint32_t f = 0;
#pragma unroll
    for (uint32_t s = 0; s < 4; ++s) f |= (oe[s & 1] | (((s >> 1) ^ qp[s & 1]) << 1)) << (8 * s);
    return f;
}

// inclusive scan of the lanes' maps over the block (sh: kBlock words); returns the lane's EXCLUSIVE prefix
__device__ __forceinline__ uint32_t block_fn_scan(uint32_t f, uint32_t* sh, uint32_t& total) {
    const uint32_t t = threadIdx.x;
    sh[t] = f;
    __syncthreads();
    for (uint32_t d = 1; d < kBlock; d <<= 1) {
        const uint32_t v = t >= d ? fn_then(sh[t - d], sh[t]) : sh[t];
        __syncthreads();
        sh[t] = v;
        __syncthreads();
    }
    total = sh[kBlock - 1];
    const uint32_t ex = t ? sh[t - 1] : kIdent;
    __syncthreads();
    return ex;
}

__global__ __launch_bounds__(kBlock) void k_tile_fn(const uint8_t* __restrict__ bytes, const ull* __restrict__ off, const uint32_t* __restrict__ tile_msg,
                                                    const ull* __restrict__ tile_at, uint32_t* __restrict__ tfn) {
    __shared__ uint32_t sh[kBlock];
    const uint32_t tile = blockIdx.x, m = tile_msg[tile];
    uint8_t b[16];
    load_chunk(bytes, tile_at[tile] + threadIdx.x * 16, off[m], off[m + 1], b);
    uint32_t total;
    (void)block_fn_scan(chunk_fn(b), sh, total);
    if (threadIdx.x == 0) {
        const bool first = tile == 0 || tile_msg[tile - 1] != m;
        tfn[tile] = first ? fn_apply(total, 0) * 0x01010101u : total;
    }
}

// one block: the state at every tile's first byte
__global__ __launch_bounds__(kBlock) void k_tile_carry(const uint32_t* __restrict__ tfn, const uint32_t* __restrict__ tile_msg, uint64_t n_tiles,
                                                       uint8_t* __restrict__ tstate) {
    __shared__ uint32_t sh[kBlock];
    const uint64_t per = (n_tiles + kBlock - 1) / kBlock;
    const uint64_t b = umin(n_tiles, threadIdx.x * per), e = umin(n_tiles, b + per);
    uint32_t f = kIdent;
    for (uint64_t i = b; i < e; ++i) f = fn_then(f, tfn[i]);
    uint32_t total;
    uint32_t s = fn_apply(block_fn_scan(f, sh, total), 0);
    for (uint64_t i = b; i < e; ++i) {
        if (i == 0 || tile_msg[i - 1] != tile_msg[i]) s = 0;
        tstate[i] = (uint8_t)s;
        s = fn_apply(tfn[i], s);
    }
}

__global__ void k_msg_init(MsgScan* ms, uint64_t n) {
    const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n) return;
    MsgScan z{};
    z.lbr_min = z.rbr_min = ~0ull;
    z.end_state = kNone;
    ms[m] = z;
}

// Every byte outside a string is checked against what a flat message may hold there, and the element starts (an
// opening quote, or the n of a null) are marked: emask bit j = byte j of the lane's chunk starts an element.
__global__ __launch_bounds__(kBlock) void k_mark(const uint8_t* __restrict__ bytes, const ull* __restrict__ off, const uint32_t* __restrict__ tile_msg,
                                                 const ull* __restrict__ tile_at, const uint8_t* __restrict__ tstate, MsgScan* __restrict__ ms,
                                                 uint16_t* __restrict__ emask, uint32_t* __restrict__ tcnt) {
    __shared__ uint32_t sh[kBlock];
    __shared__ uint32_t count;
    const uint32_t tile = blockIdx.x, m = tile_msg[tile];
    const uint64_t lo = off[m], hi = off[m + 1], at = tile_at[tile] + threadIdx.x * 16;
    if (threadIdx.x == 0) count = 0;
    uint8_t b[16];
    load_chunk(bytes, at, lo, hi, b);
    uint32_t total;
    uint32_t s = fn_apply(block_fn_scan(chunk_fn(b), sh, total), tstate[tile]);
    uint32_t esc = s & 1, inq = s >> 1, mask = 0;
    bool bad = false;
    MsgScan& M = ms[m];
    for (int j = 0; j < 16; ++j) {
        const uint64_t p = at + j;
        if (p < lo || p >= hi) continue;
        const int c = b[j];
        if (esc) {
            esc = 0;
        } else if (c == '\\') {
            esc = 1;
            bad |= !inq;
        } else if (c == '"') {
            if (!inq) mask |= 1u << j;
            inq ^= 1;
        } else if (!inq && !is_ws(c)) {
            switch (c) {
                case '[': {
                    atomicAdd(&M.n_lbr, 1u);
                    atomicMin(&M.lbr_min, (ull)p);
                    atomicMax(&M.lbr_max, (ull)p);
                    const int nx = next_token(bytes, p + 1, hi);
                    bad |= !(nx == '"' || nx == 'n' || nx == ']');
                    break;
                }
                case ']':
                    atomicAdd(&M.n_rbr, 1u);
                    atomicMin(&M.rbr_min, (ull)p);
                    atomicMax(&M.rbr_max, (ull)p);
                    break;
                case '{': atomicAdd(&M.n_lbrace, 1u); break;
                case '}': atomicAdd(&M.n_rbrace, 1u); break;
                case ':': atomicAdd(&M.n_colon, 1u); break;
                case ',': {
                    const int nx = next_token(bytes, p + 1, hi);
                    bad |= !(nx == '"' || nx == 'n');
                    break;
                }
                case 'n': mask |= 1u << j; break;  // k_strings checks the rest of the literal
                case 'u':
                case 'l': {  // only inside a null: right after its n, u or l
                    const int pv = p > lo ? bytes[p - 1] : ' ';
                    bad |= !(pv == 'n' || pv == 'u' || pv == 'l');
                    break;
                }
                default: bad = true;
            }
        }
        if (p + 1 == hi) M.end_state = esc | inq << 1;
    }
    if (bad) atomicOr(&M.notflat, 1u);
    emask[(uint64_t)tile * kBlock + threadIdx.x] = (uint16_t)mask;
    if (mask) atomicAdd(&count, (uint32_t)__popc(mask));
    __syncthreads();
    if (threadIdx.x == 0) tcnt[tile] = count;
}

// exclusive scan of n counts in one block: out[i] = in[0] + .. + in[i-1], out[n] = the total
template <class T>
__global__ __launch_bounds__(1024) void k_excl_scan(const T* __restrict__ in, ull* __restrict__ out, uint64_t n) {
    __shared__ ull sh[1024];
    const uint32_t t = threadIdx.x;
    const uint64_t per = (n + 1023) / 1024;
    const uint64_t b = umin(n, t * per), e = umin(n, b + per);
    ull sum = 0;
    for (uint64_t i = b; i < e; ++i) sum += in[i];
    sh[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const ull v = t >= d ? sh[t - d] + sh[t] : sh[t];
        __syncthreads();
        sh[t] = v;
        __syncthreads();
    }
    ull run = t ? sh[t - 1] : 0;
    for (uint64_t i = b; i < e; ++i) {
        out[i] = run;
        run += in[i];
    }
    if (t == 1023) out[n] = sh[1023];
}

// The same over many blocks, for the long arrays (one per candidate): per-block sums, the one-block scan over
// them, then each block scans its own tile from its base.  Three launches; no block waits on another.
constexpr uint32_t kScanItems = 8, kScanTile = kBlock * kScanItems;
__device__ __forceinline__ ull scan_tile_load(const uint32_t* __restrict__ in, uint64_t n, uint32_t (&v)[kScanItems]) {
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + threadIdx.x * kScanItems;
    ull s = 0;
#pragma unroll
    for (uint32_t j = 0; j < kScanItems; ++j) {
        v[j] = base + j < n ? in[base + j] : 0;
        s += v[j];
    }
    return s;
}
__global__ __launch_bounds__(kBlock) void k_scan_sum(const uint32_t* __restrict__ in, uint64_t n, ull* __restrict__ bsum) {
    __shared__ ull sh[kBlock];
    uint32_t v[kScanItems];
    sh[threadIdx.x] = scan_tile_load(in, n, v);
    __syncthreads();
    for (uint32_t d = kBlock / 2; d; d >>= 1) {
        if (threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) bsum[blockIdx.x] = sh[0];
}
__global__ __launch_bounds__(kBlock) void k_scan_apply(const uint32_t* __restrict__ in, uint64_t n, const ull* __restrict__ bbase, ull* __restrict__ out) {
    __shared__ ull sh[kBlock];
    const uint32_t t = threadIdx.x;
    uint32_t v[kScanItems];
    sh[t] = scan_tile_load(in, n, v);
    __syncthreads();
    for (uint32_t d = 1; d < kBlock; d <<= 1) {
        const ull x = t >= d ? sh[t - d] + sh[t] : sh[t];
        __syncthreads();
        sh[t] = x;
        __syncthreads();
    }
    ull run = bbase[blockIdx.x] + (t ? sh[t - 1] : 0);
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + t * kScanItems;
#pragma unroll
    for (uint32_t j = 0; j < kScanItems; ++j) {
        if (base + j < n) out[base + j] = run;
        run += v[j];
    }
    if (blockIdx.x == 0 && t == 0) out[n] = bbase[gridDim.x];
}

// element g of the call = the position of its first byte, in text order
__global__ __launch_bounds__(kBlock) void k_emit(const uint32_t* __restrict__ tile_msg, const ull* __restrict__ tile_at, const uint16_t* __restrict__ emask,
                                                 const ull* __restrict__ tbase, ull* __restrict__ epos, uint32_t* __restrict__ emsg) {
    __shared__ uint32_t sh[kBlock];
    const uint32_t tile = blockIdx.x, t = threadIdx.x;
    uint32_t mask = emask[(uint64_t)tile * kBlock + t];
    sh[t] = (uint32_t)__popc(mask);
    __syncthreads();
    for (uint32_t d = 1; d < kBlock; d <<= 1) {
        const uint32_t v = t >= d ? sh[t - d] + sh[t] : sh[t];
        __syncthreads();
        sh[t] = v;
        __syncthreads();
    }
    ull g = tbase[tile] + (t ? sh[t - 1] : 0);
    const ull at = tile_at[tile] + t * 16;
    while (mask) {
        const int j = __ffs((int)mask) - 1;
        mask &= mask - 1;
        epos[g] = at + j;
        emsg[g] = tile_msg[tile];
        ++g;
    }
}

// one lane per element: the string is well formed (read_string: escapes, surrogates, UTF-8) and what follows it is a
// separator a flat message may hold there; a null is spelled out and followed the same way
__global__ void k_strings(const uint8_t* __restrict__ bytes, const ull* __restrict__ off, const ull* __restrict__ epos, const uint32_t* __restrict__ emsg,
                          uint64_t n_elems, MsgScan* __restrict__ ms) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_elems) return;
    const uint32_t m = emsg[g];
    if (ms[m].notflat) return;
    const uint64_t p = epos[g], hi = off[m + 1];
    bool ok;
    if (bytes[p] == '"') {
        jgw::Cursor c(bytes, p + 1, hi);
        jgw::NullSink s;
        ok = jgw::read_string(c, s);
        if (ok) {
            const int nx = next_token(bytes, c.p, hi);
            ok = nx == ',' || nx == ']' || nx == ':';
        }
    } else {
        ok = p + 4 <= hi && bytes[p + 1] == 'u' && bytes[p + 2] == 'l' && bytes[p + 3] == 'l';
        if (ok) {
            const int nx = next_token(bytes, p + 4, hi);
            ok = nx == ',' || nx == ']';
        }
    }
    if (!ok) atomicOr(&ms[m].notflat, 1u);
}

__device__ __forceinline__ uint64_t lower_bound(const ull* a, uint64_t b, uint64_t e, ull v) {
    while (b < e) {
        const uint64_t mid = b + (e - b) / 2;
        if (a[mid] < v) b = mid + 1;
        else e = mid;
    }
    return b;
}

// one lane per message: its few top-level tokens.  flat[m] = 1 only when the message is proven
// ws { ws "addSet" ws : ws [ elements ] ws , ws "removeSet" ws : ws [ elements ] ws } ws — then the serial parser
// accepts it with the same elements (k_mark and k_strings proved the arrays' insides), cnt / first name them.
__global__ void k_walk(const uint8_t* __restrict__ bytes, const ull* __restrict__ off, uint64_t n, const MsgScan* __restrict__ ms,
                       const ull* __restrict__ tbase, const ull* __restrict__ msg_tile0, const ull* __restrict__ epos, uint8_t* __restrict__ flat,
                       uint32_t* __restrict__ cnt, ull* __restrict__ first, ull* __restrict__ stat) {
    const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n) return;
    flat[m] = 0;
    const MsgScan M = ms[m];
    const uint64_t lo = off[m], hi = off[m + 1];
    if (lo == hi || M.notflat || M.end_state != 0) return;
    if (M.n_lbrace != 1 || M.n_rbrace != 1 || M.n_lbr != 2 || M.n_rbr != 2 || M.n_colon != 2) return;
    if (!(M.lbr_min < M.rbr_min && M.rbr_min < M.lbr_max && M.lbr_max < M.rbr_max)) return;
    jgw::Cursor c(bytes, lo, hi);
    if (!c.expect('{') || !c.expect('"')) return;
    NameSink a;
    if (!jgw::read_string(c, a) || a.which() != 0 || !c.expect(':')) return;
    c.ws();
    if (c.p != M.lbr_min) return;
    c.p = M.rbr_min + 1;
    if (!c.expect(',') || !c.expect('"')) return;
    NameSink r;
    if (!jgw::read_string(c, r) || r.which() != 1 || !c.expect(':')) return;
    c.ws();
    if (c.p != M.lbr_max) return;
    c.p = M.rbr_max + 1;
    if (!c.expect('}')) return;
    c.ws();
    if (c.p != hi) return;
    // elements by position: exactly the two names lie outside the arrays
    const uint64_t e0 = tbase[msg_tile0[m]], e1 = tbase[msg_tile0[m + 1]];
    const uint64_t a0 = lower_bound(epos, e0, e1, M.lbr_min), a1 = lower_bound(epos, e0, e1, M.rbr_min);
    const uint64_t r0 = lower_bound(epos, e0, e1, M.lbr_max), r1 = lower_bound(epos, e0, e1, M.rbr_max);
    if (a0 - e0 != 1 || r0 - a1 != 1 || r1 != e1) return;
    flat[m] = 1;
    cnt[2 * m] = (uint32_t)(a1 - a0), cnt[2 * m + 1] = (uint32_t)(r1 - r0);
    first[2 * m] = a0, first[2 * m + 1] = r0;
    atomicAdd(&stat[0], 1ull);
    atomicAdd(&stat[1], (ull)(hi - lo));
}

// ---- serial path + candidates ---------------------------------------------------------------------
// status: 0 applies whole, 1 nothing, 2 addSet only; bad[0] = the first message with status != 0
__global__ void k_serial(const uint8_t* __restrict__ bytes, const ull* __restrict__ off, uint64_t n, const uint8_t* __restrict__ flat,
                         uint8_t* __restrict__ status, uint32_t* __restrict__ cnt, ull* __restrict__ first, ull* __restrict__ bad) {
    const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n) return;
    if (flat[m]) {
        status[m] = 0;
        return;
    }
    uint64_t pos[2] = {0, 0};
    uint32_t k[2] = {0, 0};
    const int st = parse_serial(bytes, off[m], off[m + 1], pos, k);
    status[m] = (uint8_t)st;
    cnt[2 * m] = st == 1 ? 0 : k[0];
    cnt[2 * m + 1] = st == 0 ? k[1] : 0;
    first[2 * m] = pos[0], first[2 * m + 1] = pos[1];
    if (st) atomicMin(&bad[0], (ull)m);
}

// lim[0] = first bad message (n if none), lim[1] = its status, lim[2] = candidates that apply
__global__ void k_limit(const ull* __restrict__ bad, const uint8_t* __restrict__ status, const ull* __restrict__ cbase, uint64_t n, ull* __restrict__ lim) {
    const ull b = bad[0] < n ? bad[0] : n;
    lim[0] = b;
    lim[1] = b < n ? status[b] : 0;
    lim[2] = b == n ? cbase[2 * n] : status[b] == 2 ? cbase[2 * b + 1] : cbase[2 * b];
}

// candidate slot of a flat message's element: by its rank in its array
__global__ void k_place(const ull* __restrict__ epos, const uint32_t* __restrict__ emsg, uint64_t n_elems, const uint8_t* __restrict__ flat,
                        const uint32_t* __restrict__ cnt, const ull* __restrict__ first, const ull* __restrict__ cbase, uint64_t n_cand,
                        ull* __restrict__ cpos, uint8_t* __restrict__ cwhich) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_elems) return;
    const uint32_t m = emsg[g];
    if (!flat[m]) return;
    for (uint32_t w = 0; w < 2; ++w) {
        const ull f = first[2 * m + w];
        if (g >= f && g < f + cnt[2 * m + w]) {
            const ull slot = cbase[2 * m + w] + (g - f);
            if (slot < n_cand) {
                cpos[slot] = epos[g];
                cwhich[slot] = (uint8_t)w;
            }
        }
    }
}

__global__ void k_serial_emit(const uint8_t* __restrict__ bytes, const ull* __restrict__ off, uint64_t n, const uint8_t* __restrict__ flat,
                              const uint8_t* __restrict__ status, const uint32_t* __restrict__ cnt, const ull* __restrict__ first,
                              const ull* __restrict__ cbase, uint64_t n_cand, ull* __restrict__ cpos, uint8_t* __restrict__ cwhich) {
    const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n || flat[m] || status[m] == 1) return;
    for (uint32_t w = 0; w < 2; ++w) {
        const uint32_t k = cnt[2 * m + w];
        ull slot = cbase[2 * m + w];
        if (k == 0 || slot >= n_cand) continue;
        jgw::Cursor c(bytes, first[2 * m + w], off[m + 1]);
        for (uint32_t i = 0; i < k && slot < n_cand; ++i, ++slot) {  // the walk k_serial validated
            c.ws();
            cpos[slot] = c.p;
            cwhich[slot] = (uint8_t)w;
            if (c.peek() == '"') {
                ++c.p;
                jgw::NullSink s;
                (void)jgw::read_string(c, s);
            } else {
                c.p += 4;
            }
            c.ws();
            ++c.p;  // ',' or ']'
        }
    }
}

// A candidate: string bytes tmp[cstart, cstart + clen), key ckey, cwhich bit 0 = removeSet, bit 1 = the null element.
// From JSON: the string is unescaped in place behind its opening quote (never longer than its escaped form).
__global__ void k_cand_hash(const uint8_t* __restrict__ bytes, uint64_t n_bytes, uint8_t* __restrict__ tmp, const ull* __restrict__ cpos, uint64_t n_cand,
                            uint64_t salt, ull* __restrict__ cstart, uint32_t* __restrict__ clen, ull* __restrict__ ckey, uint8_t* __restrict__ cwhich) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cand) return;
    const uint64_t p = cpos[c];
    cstart[c] = p + 1;
    if (bytes[p] != '"') {
        cwhich[c] |= 2;
        clen[c] = 0;
        ckey[c] = 0;
        return;
    }
    jgw::Cursor cur(bytes, p + 1, n_bytes);
    HashSink s{tmp + p + 1};
    (void)jgw::read_string(cur, s);  // validated by k_strings / k_serial
    clen[c] = s.n;
    ckey[c] = str_key(s.h, salt);
}

// the same for strings given raw (jg_tpset_apply_ops / _contains): string i = tmp[off[i], off[i+1])
__global__ void k_raw_hash(const uint8_t* __restrict__ tmp, const ull* __restrict__ off, const uint8_t* __restrict__ op, const uint8_t* __restrict__ is_null,
                           uint64_t n, uint64_t salt, ull* __restrict__ cstart, uint32_t* __restrict__ clen, ull* __restrict__ ckey,
                           uint8_t* __restrict__ cwhich) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const bool nul = is_null && is_null[c];
    const uint32_t len = nul ? 0 : (uint32_t)(off[c + 1] - off[c]);
    uint64_t h = kFnvBasis;
    for (uint32_t i = 0; i < len; ++i) h = (h ^ tmp[off[c] + i]) * kFnvPrime;
    cstart[c] = off[c];
    clen[c] = len;
    ckey[c] = nul ? 0 : str_key(h, salt);
    cwhich[c] = (uint8_t)((op ? op[c] - 1 : 0) | (nul ? 2 : 0));
}

struct Cands {
    const uint8_t* tmp;
    ull* cstart;
    uint32_t* clen;
    ull* ckey;
    uint8_t* cwhich;
    uint32_t* cres;   // resident string id, kNone
    uint32_t* cslot;  // slot of the call-wide table, kNone = nothing to insert
    uint32_t* prep;   // call-wide table: a candidate holding the slot's string, + 1 (0 = empty)
    uint32_t* pmin;   // [2 x slots]: the first candidate adding the string to add[] / rem[]
    uint32_t* newid;  // [slots]: the id a new string took
    uint32_t* nullmin;  // [2] the same for the null element
    uint64_t pmask;
    uint64_t n;
};

// slot of candidate c's string in the call-wide table (inserted if absent).  A lost CAS is answered by the value it
// returned, never by waiting: the slot then holds some candidate's string, equal to this one or not.
__device__ uint32_t cand_slot(const Cands& K, uint64_t c) {
    const uint8_t* s = K.tmp + K.cstart[c];
    const uint32_t len = K.clen[c];
    const ull key = K.ckey[c];
    for (uint64_t slot = key & K.pmask;; slot = (slot + 1) & K.pmask) {
        uint32_t r = K.prep[slot];
        if (r == 0) {
            r = atomicCAS(&K.prep[slot], 0u, (uint32_t)c + 1);
            if (r == 0) return (uint32_t)slot;
        }
        const uint32_t o = r - 1;
        if (K.ckey[o] == key && K.clen[o] == len && same_bytes(K.tmp + K.cstart[o], s, len)) return (uint32_t)slot;
    }
}

// ops = 0 (merge): every candidate whose string its array lacks bids for the string's first place in that array.
// ops = 1 (apply_ops): only the Adds bid here; the Removes bid in k_ops_remove, once the Adds' minima stand.
__global__ void k_cand_find(Store S, Cands K, int ops) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= K.n) return;
    const uint32_t w = K.cwhich[c] & 1;
    K.cslot[c] = kNone;
    K.cres[c] = kNone;
    if (K.cwhich[c] & 2) {
        if (S.nulls[w] == kNone && !(ops && w)) atomicMin(&K.nullmin[w], (uint32_t)c);
        return;
    }
    const uint32_t id = store_find(S, K.ckey[c], K.tmp + K.cstart[c], K.clen[c]);
    K.cres[c] = id;
    const bool have = id != kNone && (w ? S.srem[id] : S.sadd[id]) != kNone;
    if (have && !ops) return;
    const uint32_t slot = cand_slot(K, c);
    K.cslot[c] = slot;
    if (!have && !(ops && w)) atomicMin(&K.pmin[w * (K.pmask + 1) + slot], (uint32_t)c);
}

// TPSet.Remove (2P-Set.cs:117-126) for a batch in op order: Remove i finds its string present iff the string is in
// addSet by then (resident, or an Add of the batch before i) and not in removeSet (resident, or an earlier Remove of
// the batch that found it present).  So exactly the first Remove after the string's first Add succeeds.
__global__ void k_ops_remove(Store S, Cands K) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= K.n || !(K.cwhich[c] & 1)) return;
    if (K.cwhich[c] & 2) {
        if (S.nulls[1] != kNone) return;
        if (S.nulls[0] != kNone || K.nullmin[0] < c) atomicMin(&K.nullmin[1], (uint32_t)c);
        return;
    }
    const uint32_t id = K.cres[c], slot = K.cslot[c];
    if (id != kNone && S.srem[id] != kNone) return;
    if ((id != kNone && S.sadd[id] != kNone) || K.pmin[slot] < c) atomicMin(&K.pmin[K.pmask + 1 + slot], (uint32_t)c);
}

// winners: wa / wr = the candidate appends its string to add[] / rem[]; ws = it also brings the string's bytes.
// The bytes of a new string come from the slot's representative, the candidate that won cand_slot's CAS, which need
// not be the first occurrence: string ids and the pool's layout may differ from run to run and are NOT insertion
// order; only the ordinals in add[] / rem[] are, and nothing observable reads the pool's order.  newid[] is never
// cleared: a winner with cres == kNone reads newid[its slot], and that slot's representative has ws set exactly
// when some candidate of the slot wins (pmin of the slot is set), so the entry is written before it is read.
__global__ void k_cand_win(Cands K, uint32_t* __restrict__ wa, uint32_t* __restrict__ wr, uint32_t* __restrict__ ws, uint32_t* __restrict__ wb,
                           uint8_t* __restrict__ result) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= K.n) return;
    const uint32_t w = K.cwhich[c] & 1;
    bool win, str = false;
    if (K.cwhich[c] & 2) {
        win = K.nullmin[w] == c;
    } else {
        const uint32_t slot = K.cslot[c];
        win = slot != kNone && K.pmin[w * (K.pmask + 1) + slot] == c;
        str = slot != kNone && K.cres[c] == kNone && K.prep[slot] == c + 1 && (K.pmin[slot] != kNone || K.pmin[K.pmask + 1 + slot] != kNone);
    }
    wa[c] = win && !w, wr[c] = win && w, ws[c] = str, wb[c] = str ? K.clen[c] : 0;
    if (result) result[c] = w ? win : 1;  // Add returns nothing: 1; Remove its bool
}

__global__ void k_commit_strings(Store S, Cands K, const uint32_t* __restrict__ ws, const ull* __restrict__ os, const ull* __restrict__ ob, uint64_t n_str,
                                 uint64_t n_bytes) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= K.n || !ws[c]) return;
    const uint32_t id = (uint32_t)(n_str + os[c]);
    const ull at = n_bytes + ob[c];
    const uint32_t len = K.clen[c];
    const uint8_t* s = K.tmp + K.cstart[c];
    for (uint32_t i = 0; i < len; ++i) S.pool[at + i] = s[i];
    S.soff[id] = at, S.slen[id] = len, S.skey[id] = K.ckey[c], S.sadd[id] = kNone, S.srem[id] = kNone;
    K.newid[K.cslot[c]] = id;
    for (uint64_t slot = K.ckey[c] & S.tmask;; slot = (slot + 1) & S.tmask)  // the table is at most half full
        if (S.table[slot] == 0 && atomicCAS(&S.table[slot], 0u, id + 1) == 0) break;
}

__global__ void k_commit_entries(Store S, Cands K, const uint32_t* __restrict__ wa, const uint32_t* __restrict__ wr, const ull* __restrict__ oa,
                                 const ull* __restrict__ orr, uint64_t n_add, uint64_t n_rem) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= K.n || !(wa[c] | wr[c])) return;
    const bool w = wr[c];
    const uint32_t ord = (uint32_t)(w ? n_rem + orr[c] : n_add + oa[c]);
    uint32_t id;
    if (K.cwhich[c] & 2) {
        id = kNullId;
        S.nulls[w] = ord;
    } else {
        id = K.cres[c] != kNone ? K.cres[c] : K.newid[K.cslot[c]];
        (w ? S.srem : S.sadd)[id] = ord;
    }
    (w ? S.rem : S.add)[ord] = id;
}

// ---- queries ---------------------------------------------------------------------------------------
// TPSet.Contains (2P-Set.cs:169-172)
__global__ void k_contains(Store S, Cands K, uint8_t* __restrict__ out) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= K.n) return;
    if (K.cwhich[c] & 2) {
        out[c] = S.nulls[0] != kNone && S.nulls[1] == kNone;
        return;
    }
    const uint32_t id = store_find(S, K.ckey[c], K.tmp + K.cstart[c], K.clen[c]);
    out[c] = id != kNone && S.sadd[id] != kNone && S.srem[id] == kNone;
}

// TPSet.LookupAll (2P-Set.cs:133-136): addSet.Except(removeSet) from ordinal `from` on
__global__ void k_lookup_flag(Store S, uint64_t from, uint64_t n, uint32_t* __restrict__ keep, uint32_t* __restrict__ len) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t id = S.add[from + i];
    const bool k = id == kNullId ? S.nulls[1] == kNone : S.srem[id] == kNone;
    keep[i] = k;
    len[i] = k && id != kNullId ? S.slen[id] : 0;
}
__global__ void k_lookup_write(Store S, uint64_t from, uint64_t n, const uint32_t* __restrict__ keep, const ull* __restrict__ ok, const ull* __restrict__ ob,
                               ull* __restrict__ ord, ull* __restrict__ off, uint8_t* __restrict__ bytes, uint8_t* __restrict__ is_null) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) off[ok[n]] = ob[n];
    if (i >= n || !keep[i]) return;
    const uint32_t id = S.add[from + i];
    const ull k = ok[i];
    ord[k] = from + i;
    off[k] = ob[i];
    is_null[k] = id == kNullId;
    if (id == kNullId) return;
    const uint8_t* s = S.pool + S.soff[id];
    for (uint32_t j = 0, l = S.slen[id]; j < l; ++j) bytes[ob[i] + j] = s[j];
}

// ---- encode: TPSetMsg.Encode() (2P-Set.cs:49-52) of the whole set ---------------------------------
// JavaScriptEncoder.Default (oracle/json.hpp EscapeTo): the wire bytes of the UTF-8 sequence at s into w (at most 12),
// their count returned, adv = the sequence's length.  The one definition both the length and the write pass use.
__device__ __forceinline__ void put_u16(uint8_t* o, uint32_t u) {
    const char* HX = "0123456789ABCDEF";
    o[0] = '\\', o[1] = 'u', o[2] = HX[(u >> 12) & 15], o[3] = HX[(u >> 8) & 15], o[4] = HX[(u >> 4) & 15], o[5] = HX[u & 15];
}
__device__ __forceinline__ uint32_t esc_seq(const uint8_t* s, uint32_t& adv, uint8_t (&w)[12]) {
    const uint8_t c = s[0];
    if (c < 0x80) {
        adv = 1;
        const int two = c == '\\' ? '\\' : c == '\b' ? 'b' : c == '\t' ? 't' : c == '\n' ? 'n' : c == '\f' ? 'f' : c == '\r' ? 'r' : 0;
        if (two) {
            w[0] = '\\', w[1] = (uint8_t)two;
            return 2;
        }
        if (c < 0x20 || c == 0x7F || c == '"' || c == '&' || c == '\'' || c == '+' || c == '<' || c == '>' || c == '`') {
            put_u16(w, c);
            return 6;
        }
        w[0] = c;
        return 1;
    }
    adv = (c & 0xE0) == 0xC0 ? 2 : (c & 0xF0) == 0xE0 ? 3 : 4;
    uint32_t cp = c & (adv == 2 ? 0x1F : adv == 3 ? 0x0F : 0x07);
    for (uint32_t k = 1; k < adv; ++k) cp = cp << 6 | (s[k] & 0x3F);
    if (cp < 0x10000) {
        put_u16(w, cp);
        return 6;
    }
    cp -= 0x10000;
    put_u16(w, 0xD800 | (cp >> 10));
    put_u16(w + 6, 0xDC00 | (cp & 0x3FF));
    return 12;
}
// Entry e of add[] followed by rem[] owns one piece of the wire form: what separates it from the entry before (the
// head and / or the member name in front of an array's first entry, else a comma), its element, and behind the last
// entry whatever closes the message.  The pieces tile the output, so eo[] (the scan of their lengths) holds absolute
// offsets and eo[n_add + n_rem] the message's length.
__device__ __forceinline__ void enc_lits(uint64_t e, uint64_t n_add, uint64_t n_rem, uint8_t (&pre)[26], uint32_t& np, uint8_t (&suf)[17], uint32_t& ns) {
    const char* H = "{\"addSet\":[";
    const char* M = "],\"removeSet\":[";
    np = ns = 0;
    if (e == 0)
        for (uint32_t i = 0; i < 11; ++i) pre[np++] = H[i];
    if (e == n_add)
        for (uint32_t i = 0; i < 15; ++i) pre[np++] = M[i];
    else if (e != 0)
        pre[np++] = ',';
    if (e + 1 == n_add + n_rem) {
        if (n_rem == 0)
            for (uint32_t i = 0; i < 15; ++i) suf[ns++] = M[i];
        suf[ns++] = ']', suf[ns++] = '}';
    }
}
__global__ void k_enc_len(Store S, uint64_t n_add, uint64_t n_rem, uint32_t* __restrict__ len) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_add + n_rem) return;
    const uint32_t id = e < n_add ? S.add[e] : S.rem[e - n_add];
    uint8_t pre[26], suf[17];
    uint32_t np, ns;
    enc_lits(e, n_add, n_rem, pre, np, suf, ns);
    uint32_t l = np + ns;
    if (id == kNullId) {
        l += 4;
    } else {
        l += 2;
        const uint8_t* s = S.pool + S.soff[id];
        uint8_t w[12];
        for (uint32_t i = 0, n = S.slen[id], adv; i < n; i += adv) l += esc_seq(s + i, adv, w);
    }
    len[e] = l;
}

// The write pass, staged as pnc_encode.hip's: a block's 256 pieces are contiguous on the wire, so its lanes write their
// bytes into an LDS window of kStage bytes (aligned to 16 in output coordinates) and the block then stores the window
// as whole 16-byte chunks, bytes only at the two ragged ends it shares with its neighbours.  A block whose pieces
// run past one window (a long string, or just 256 long entries) takes window after window: a lane keeps its place
// in its string (i, and bp = where s[i]'s escape starts on the wire) and an escape that straddles two windows is
// produced in both, each keeping its own bytes.
constexpr uint32_t kStage = 16384;
__global__ __launch_bounds__(kBlock) void k_enc_write(Store S, uint64_t n_add, uint64_t n_rem, const ull* __restrict__ eo, uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[kStage];
    const uint32_t t = threadIdx.x;
    const uint64_t ne = n_add + n_rem, e0 = (uint64_t)blockIdx.x * kBlock, e = e0 + t, e1 = umin(ne, e0 + kBlock);
    const ull A = eo[e0], B = eo[e1];
    const bool live = e < ne;
    ull beg = 0, end = 0, body = 0, bp = 0;
    uint8_t pre[26], suf[17];
    uint32_t np = 0, ns = 0, id = kNullId, i = 0, n = 0;
    const uint8_t* s = nullptr;
    if (live) {
        beg = eo[e], end = eo[e + 1];
        enc_lits(e, n_add, n_rem, pre, np, suf, ns);
        id = e < n_add ? S.add[e] : S.rem[e - n_add];
        body = beg + np, bp = body + 1;
        if (id != kNullId) s = S.pool + S.soff[id], n = S.slen[id];
    }
    for (ull w = A & ~15ull; w < B; w += kStage) {
        const ull wend = w + kStage;
        if (live && beg < wend && end > w) {
            auto put = [&](ull p, uint8_t b) {
                if (p >= w && p < wend) stage[p - w] = b;
            };
            for (uint32_t j = 0; j < np; ++j) put(beg + j, pre[j]);
            if (id == kNullId) {
                put(body, 'n'), put(body + 1, 'u'), put(body + 2, 'l'), put(body + 3, 'l');
            } else {
                put(body, '"');
                while (i < n && bp < wend) {
                    uint8_t wb[12];
                    uint32_t adv;
                    const uint32_t k = esc_seq(s + i, adv, wb);
                    for (uint32_t j = 0; j < k; ++j) put(bp + j, wb[j]);
                    if (bp + k > wend) break;  // the rest of this escape belongs to the next window
                    bp += k, i += adv;
                }
                put(end - ns - 1, '"');
            }
            for (uint32_t j = 0; j < ns; ++j) put(end - ns + j, suf[j]);
        }
        __syncthreads();
        const ull lo = w > A ? w : A, hi = wend < B ? wend : B;
        const ull clo = (lo + 15) & ~15ull, chi = hi & ~15ull;
        if (clo < chi) {
            for (ull c = clo + t * 16; c < chi; c += kBlock * 16) *reinterpret_cast<uint4*>(out + c) = *reinterpret_cast<const uint4*>(stage + (c - w));
            for (ull p = lo + t; p < clo; p += kBlock) out[p] = stage[p - w];
            for (ull p = chi + t; p < hi; p += kBlock) out[p] = stage[p - w];
        } else {
            for (ull p = lo + t; p < hi; p += kBlock) out[p] = stage[p - w];
        }
        __syncthreads();
    }
}

// well-formed UTF-8 (what a C# string encodes to): the encoder walks sequences by their lead byte
bool valid_utf8(const uint8_t* s, uint64_t n) {
    for (uint64_t i = 0; i < n;) {
        const uint8_t c = s[i];
        if (c < 0x80) {
            ++i;
            continue;
        }
        uint32_t len, cp;
        if (c >= 0xC2 && c <= 0xDF) len = 2, cp = c & 0x1F;
        else if (c >= 0xE0 && c <= 0xEF) len = 3, cp = c & 0x0F;
        else if (c >= 0xF0 && c <= 0xF4) len = 4, cp = c & 0x07;
        else return false;
        if (i + len > n) return false;
        for (uint32_t k = 1; k < len; ++k) {
            if ((s[i + k] & 0xC0) != 0x80) return false;
            cp = cp << 6 | (s[i + k] & 0x3F);
        }
        if ((len == 3 && (cp < 0x800 || (cp >= 0xD800 && cp <= 0xDFFF))) || (len == 4 && (cp < 0x10000 || cp > 0x10FFFF))) return false;
        i += len;
    }
    return true;
}

void* work(jg_tpset* s, jg::DevBuf& b, size_t bytes) {
    if (b.bytes < bytes) {
        JG_HIP(hipStreamSynchronize(s->ctx->stream));
        b.alloc(bytes + bytes / 4 + 4096);
    }
    return b.p;
}

// out[0..n] = exclusive scan of in[0..n) on the set's stream
void excl_scan(jg_tpset* s, const uint32_t* in, ull* out, uint64_t n) {
    hipStream_t st = s->ctx->stream;
    if (n <= 4 * kScanTile) {
        hipLaunchKernelGGL(k_excl_scan<uint32_t>, dim3(1), dim3(1024), 0, st, in, out, n);
        return;
    }
    const uint64_t nb = (n + kScanTile - 1) / kScanTile;
    ull* bsum = static_cast<ull*>(work(s, s->wscan, (2 * nb + 2) * sizeof(ull)));
    ull* bbase = bsum + nb;
    hipLaunchKernelGGL(k_scan_sum, dim3((unsigned)nb), dim3(kBlock), 0, st, in, n, bsum);
    hipLaunchKernelGGL(k_excl_scan<ull>, dim3(1), dim3(1024), 0, st, (const ull*)bsum, bbase, nb);
    hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)nb), dim3(kBlock), 0, st, in, n, (const ull*)bbase, out);
}

template <class T> T pin_read(jg_ctx* ctx, const T* d) {  // one small synchronous read
    jg::pin_get(ctx, 0, d, sizeof(T));
    jg::pin_sync(ctx);
    return *static_cast<const T*>(jg::pin_at(ctx, 0));
}

void check_offsets(const char* fn, uint64_t n, const uint64_t* off, const uint8_t* bytes) {
    JG_REQUIRE(n == 0 || off, JG_EINVAL, "%s: off is NULL", fn);
    if (n == 0) return;
    JG_REQUIRE(off[0] == 0, JG_EINVAL, "%s: off[0] must be 0", fn);
    for (uint64_t i = 0; i < n; ++i) JG_REQUIRE(off[i] <= off[i + 1], JG_EINVAL, "%s: offsets decrease at %llu", fn, (ull)i);
    JG_REQUIRE(off[n] == 0 || bytes, JG_EINVAL, "%s: bytes is NULL", fn);
    JG_REQUIRE(n < 0xFFFFFFF0ull && off[n] < (1ull << 40), JG_EINVAL, "%s: batch too large", fn);
}

// Candidates [0, C) hashed in w3 (cstart / clen / ckey / cwhich filled): resolve them against the store and append
// the winners.  ops: the batch is jg_tpset_apply_ops' (result = the ops' bools).  JG_ESTATE before anything changes
// when the store lacks room.  Returns the entries appended.
struct CandBufs {
    Cands K;
    uint32_t *wa, *wr, *ws, *wb;
    ull *oa, *orr, *os, *ob;
    uint8_t* result;
};
void cand_layout(jg::Layout& cv, uint64_t C, CandBufs& B) {
    uint64_t slots = 64;
    while (slots < 2 * C) slots <<= 1;
    Cands& K = B.K;
    cv.add<ull>(K.cstart, C), cv.add<uint32_t>(K.clen, C), cv.add<ull>(K.ckey, C), cv.add<uint8_t>(K.cwhich, C);
    cv.add<uint32_t>(K.cres, C), cv.add<uint32_t>(K.cslot, C);
    cv.add<uint32_t>(K.prep, slots), cv.add<uint32_t>(K.pmin, 2 * slots), cv.add<uint32_t>(K.newid, slots), cv.add<uint32_t>(K.nullmin, 2);
    K.pmask = slots - 1, K.n = C;
    cv.add<uint32_t>(B.wa, C), cv.add<uint32_t>(B.wr, C), cv.add<uint32_t>(B.ws, C), cv.add<uint32_t>(B.wb, C);
    cv.add<ull>(B.oa, C + 1), cv.add<ull>(B.orr, C + 1), cv.add<ull>(B.os, C + 1), cv.add<ull>(B.ob, C + 1);
    cv.add<uint8_t>(B.result, C);
}

uint64_t insert_candidates(jg_tpset* s, CandBufs& B, bool ops, const char* fn) {
    jg_ctx* ctx = s->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t C = B.K.n, slots = B.K.pmask + 1;
    const Store S = s->view();
    JG_HIP(hipMemsetAsync(B.K.prep, 0, slots * 4, st));
    JG_HIP(hipMemsetAsync(B.K.pmin, 0xFF, 2 * slots * 4, st));
    JG_HIP(hipMemsetAsync(B.K.nullmin, 0xFF, 8, st));
    const unsigned g = blocks_for(C);
    hipLaunchKernelGGL(k_cand_find, dim3(g), dim3(kBlock), 0, st, S, B.K, ops ? 1 : 0);
    if (ops) hipLaunchKernelGGL(k_ops_remove, dim3(g), dim3(kBlock), 0, st, S, B.K);
    hipLaunchKernelGGL(k_cand_win, dim3(g), dim3(kBlock), 0, st, B.K, B.wa, B.wr, B.ws, B.wb, ops ? B.result : (uint8_t*)nullptr);
    excl_scan(s, B.wa, B.oa, C);
    excl_scan(s, B.wr, B.orr, C);
    excl_scan(s, B.ws, B.os, C);
    excl_scan(s, B.wb, B.ob, C);
    JG_HIP(hipGetLastError());
    jg::pin_get(ctx, 0, B.oa + C, 8);
    jg::pin_get(ctx, 8, B.orr + C, 8);
    jg::pin_get(ctx, 16, B.os + C, 8);
    jg::pin_get(ctx, 24, B.ob + C, 8);
    jg::pin_sync(ctx);
    const uint64_t* tot = static_cast<const uint64_t*>(jg::pin_at(ctx, 0));
    const uint64_t ta = tot[0], tr = tot[1], ts = tot[2], tb = tot[3];
    JG_REQUIRE(s->n_str + ts <= s->cap_strings, JG_ESTATE, "%s: %llu strings exceed the set's capacity of %llu (nothing applied)", fn,
               (ull)(s->n_str + ts), (ull)s->cap_strings);
    JG_REQUIRE(s->n_bytes + tb <= s->cap_bytes, JG_ESTATE, "%s: %llu string bytes exceed the set's capacity of %llu (nothing applied)", fn,
               (ull)(s->n_bytes + tb), (ull)s->cap_bytes);
    if (ta + tr) {
        hipLaunchKernelGGL(k_commit_strings, dim3(g), dim3(kBlock), 0, st, S, B.K, B.ws, B.os, B.ob, s->n_str, s->n_bytes);
        hipLaunchKernelGGL(k_commit_entries, dim3(g), dim3(kBlock), 0, st, S, B.K, B.wa, B.wr, B.oa, B.orr, s->n_add, s->n_rem);
        JG_HIP(hipGetLastError());
    }
    s->n_str += ts, s->n_bytes += tb, s->n_add += ta, s->n_rem += tr;
    return ta + tr;
}

// raw strings (apply_ops / contains) uploaded and hashed into candidate buffers
void raw_candidates(jg_tpset* s, const char* fn, uint64_t n, const uint8_t* op, const uint64_t* off, const uint8_t* bytes, const uint8_t* is_null,
                    CandBufs& B) {
    jg_ctx* ctx = s->ctx;
    hipStream_t st = ctx->stream;
    check_offsets(fn, n, off, bytes);
    for (uint64_t i = 0; i < n; ++i) {
        if (is_null && is_null[i]) continue;
        JG_REQUIRE(off[i + 1] - off[i] < (1ull << 31), JG_EINVAL, "%s: string %llu too long", fn, (ull)i);
        JG_REQUIRE(valid_utf8(bytes + off[i], off[i + 1] - off[i]), JG_EINVAL, "%s: string %llu is not well-formed UTF-8", fn, (ull)i);
    }
    const uint64_t nb = off[n];
    uint8_t* d_bytes = nullptr;
    ull* d_off = nullptr;
    uint8_t *d_op = nullptr, *d_null = nullptr;
    jg::Layout cv;
    cv.add<uint8_t>(d_bytes, nb + 64), cv.add<ull>(d_off, n + 1), cv.add<uint8_t>(d_op, n), cv.add<uint8_t>(d_null, n);
    cand_layout(cv, n, B);
    cv.bind(work(s, s->w3, cv.bytes() + 1024));
    if (nb) JG_HIP(hipMemcpyAsync(d_bytes, bytes, nb, hipMemcpyHostToDevice, st));
    JG_HIP(hipMemcpyAsync(d_off, off, (n + 1) * 8, hipMemcpyHostToDevice, st));
    if (op) JG_HIP(hipMemcpyAsync(d_op, op, n, hipMemcpyHostToDevice, st));
    if (is_null) JG_HIP(hipMemcpyAsync(d_null, is_null, n, hipMemcpyHostToDevice, st));
    B.K.tmp = d_bytes;
    hipLaunchKernelGGL(k_raw_hash, dim3(blocks_for(n)), dim3(kBlock), 0, st, d_bytes, d_off, op ? d_op : (const uint8_t*)nullptr,
                       is_null ? d_null : (const uint8_t*)nullptr, n, s->salt, B.K.cstart, B.K.clen, B.K.ckey, B.K.cwhich);
    JG_HIP(hipGetLastError());
}

}  // namespace

extern "C" {

int jg_tpset_create(jg_ctx* ctx, uint64_t cap_strings, uint64_t cap_bytes, jg_tpset** out) {
    return jg::guard([&] {
        auto lk_ = jg::lock(ctx);
        JG_REQUIRE(ctx && out, JG_EINVAL, "jg_tpset_create: NULL argument");
        JG_REQUIRE(cap_strings < 0x7FFFFFF0ull && cap_bytes < (1ull << 40), JG_EINVAL, "jg_tpset_create: capacity too large");
        jg::ensure_device(ctx);
        std::unique_ptr<jg_tpset> s(new jg_tpset());
        s->ctx = ctx;
        s->cap_strings = cap_strings, s->cap_bytes = cap_bytes;
        uint64_t slots = 64;
        while (slots < 2 * cap_strings) slots <<= 1;
        s->tmask = slots - 1;
        std::random_device rd;
        s->salt = ((uint64_t)rd() << 32 ^ rd()) | 1;
        const uint64_t n = cap_strings + 1;
        s->pool.alloc(cap_bytes + 64), s->soff.alloc(n * 8), s->slen.alloc(n * 4), s->sadd.alloc(n * 4), s->srem.alloc(n * 4), s->skey.alloc(n * 8);
        s->table.alloc(slots * 4), s->add.alloc(n * 4), s->rem.alloc(n * 4), s->nulls.alloc(8);
        JG_HIP(hipMemsetAsync(s->table.p, 0, slots * 4, ctx->stream));
        JG_HIP(hipMemsetAsync(s->nulls.p, 0xFF, 8, ctx->stream));
        JG_HIP(hipEventCreate(&s->ev0));
        JG_HIP(hipEventCreate(&s->ev1));
        JG_HIP(hipStreamSynchronize(ctx->stream));
        *out = s.release();
    });
}

int jg_tpset_destroy(jg_tpset* s) {
    return jg::guard([&] {
        if (!s) return;
        {
            auto lk_ = jg::lock(s);
            jg::ensure_device(s->ctx);
            (void)hipStreamSynchronize(s->ctx->stream);
        }
        delete s;
    });
}

int jg_tpset_size(jg_tpset* s, uint64_t* n_add, uint64_t* n_rem, uint64_t* n_bytes) {
    return jg::guard([&] {
        auto lk_ = jg::lock(s);
        JG_REQUIRE(s, JG_EINVAL, "jg_tpset_size: set is NULL");
        if (n_add) *n_add = s->n_add;
        if (n_rem) *n_rem = s->n_rem;
        if (n_bytes) *n_bytes = s->n_bytes;
    });
}

int jg_tpset_apply_ops(jg_tpset* s, uint64_t n, const uint8_t* op, const uint64_t* off, const uint8_t* bytes, const uint8_t* is_null, uint8_t* result) {
    return jg::guard([&] {
        auto lk_ = jg::lock(s);
        JG_REQUIRE(s && (n == 0 || op), JG_EINVAL, "jg_tpset_apply_ops: NULL argument");
        for (uint64_t i = 0; i < n; ++i) JG_REQUIRE(op[i] == 1 || op[i] == 2, JG_EINVAL, "jg_tpset_apply_ops: op %llu has id %u", (ull)i, op[i]);
        if (n == 0) return;
        jg::ensure_device(s->ctx);
        CandBufs B{};
        raw_candidates(s, "jg_tpset_apply_ops", n, op, off, bytes, is_null, B);
        insert_candidates(s, B, true, "jg_tpset_apply_ops");
        if (result) JG_HIP(hipMemcpyAsync(result, B.result, n, hipMemcpyDeviceToHost, s->ctx->stream));
        JG_HIP(hipStreamSynchronize(s->ctx->stream));
    });
}

int jg_tpset_contains(jg_tpset* s, uint64_t n, const uint64_t* off, const uint8_t* bytes, const uint8_t* is_null, uint8_t* out) {
    return jg::guard([&] {
        auto lk_ = jg::lock(s);
        JG_REQUIRE(s && (n == 0 || out), JG_EINVAL, "jg_tpset_contains: NULL argument");
        if (n == 0) return;
        jg::ensure_device(s->ctx);
        CandBufs B{};
        raw_candidates(s, "jg_tpset_contains", n, nullptr, off, bytes, is_null, B);
        hipLaunchKernelGGL(k_contains, dim3(blocks_for(n)), dim3(kBlock), 0, s->ctx->stream, s->view(), B.K, B.result);
        JG_HIP(hipGetLastError());
        JG_HIP(hipMemcpyAsync(out, B.result, n, hipMemcpyDeviceToHost, s->ctx->stream));
        JG_HIP(hipStreamSynchronize(s->ctx->stream));
    });
}

int jg_tpset_lookup_all(jg_tpset* s, uint64_t from_ord, uint64_t* n, uint64_t* n_bytes, uint64_t* ord, uint64_t* off, uint8_t* bytes, uint8_t* is_null) {
    return jg::guard([&] {
        auto lk_ = jg::lock(s);
        JG_REQUIRE(s && n && n_bytes, JG_EINVAL, "jg_tpset_lookup_all: NULL argument");
        const bool query = !ord && !off && !bytes && !is_null;
        JG_REQUIRE(query || (ord && off && is_null), JG_EINVAL, "jg_tpset_lookup_all: ord, off, is_null: all or none");
        jg_ctx* ctx = s->ctx;
        hipStream_t st = ctx->stream;
        jg::ensure_device(ctx);
        const uint64_t from = std::min(from_ord, s->n_add), m = s->n_add - from;
        if (m == 0) {
            *n = *n_bytes = 0;
            if (off) off[0] = 0;
            return;
        }
        uint32_t *keep = nullptr, *len = nullptr;
        ull *ok = nullptr, *ob = nullptr, *d_ord = nullptr, *d_off = nullptr;
        uint8_t *d_null = nullptr, *d_bytes = nullptr;
        const uint64_t maxb = s->n_bytes;
        jg::Layout cv;
        cv.add<uint32_t>(keep, m), cv.add<uint32_t>(len, m), cv.add<ull>(ok, m + 1), cv.add<ull>(ob, m + 1);
        cv.add<ull>(d_ord, m), cv.add<ull>(d_off, m + 1), cv.add<uint8_t>(d_null, m), cv.add<uint8_t>(d_bytes, maxb + 16);
        cv.bind(work(s, s->w3, cv.bytes() + 1024));
        const Store S = s->view();
        hipLaunchKernelGGL(k_lookup_flag, dim3(blocks_for(m)), dim3(kBlock), 0, st, S, from, m, keep, len);
        excl_scan(s, keep, ok, m);
        excl_scan(s, len, ob, m);
        if (!query) hipLaunchKernelGGL(k_lookup_write, dim3(blocks_for(m)), dim3(kBlock), 0, st, S, from, m, keep, ok, ob, d_ord, d_off, d_bytes, d_null);
        JG_HIP(hipGetLastError());
        jg::pin_get(ctx, 0, ok + m, 8);
        jg::pin_get(ctx, 8, ob + m, 8);
        jg::pin_sync(ctx);
        const uint64_t k = static_cast<const uint64_t*>(jg::pin_at(ctx, 0))[0], kb = static_cast<const uint64_t*>(jg::pin_at(ctx, 0))[1];
        const uint64_t cap_n = *n, cap_b = *n_bytes;
        *n = k, *n_bytes = kb;
        if (query) return;
        JG_REQUIRE(k <= cap_n && kb <= cap_b && (kb == 0 || bytes), JG_ESTATE, "jg_tpset_lookup_all: %llu strings / %llu bytes exceed the buffers", (ull)k,
                   (ull)kb);
        JG_HIP(hipMemcpyAsync(off, d_off, (k + 1) * 8, hipMemcpyDeviceToHost, st));
        if (k) JG_HIP(hipMemcpyAsync(ord, d_ord, k * 8, hipMemcpyDeviceToHost, st));
        if (k) JG_HIP(hipMemcpyAsync(is_null, d_null, k, hipMemcpyDeviceToHost, st));
        if (kb) JG_HIP(hipMemcpyAsync(bytes, d_bytes, kb, hipMemcpyDeviceToHost, st));
        JG_HIP(hipStreamSynchronize(st));
    });
}

int jg_tpset_merge_json(jg_tpset* s, uint64_t n, const uint64_t* off, const uint8_t* bytes, uint32_t mode, uint64_t* bad_msg, uint8_t* partial) {
    if (bad_msg) *bad_msg = UINT64_MAX;
    if (partial) *partial = 0;
    return jg::guard([&] {
        auto lk_ = jg::lock(s);
        JG_REQUIRE(s, JG_EINVAL, "jg_tpset_merge_json: set is NULL");
        JG_REQUIRE(mode <= 1, JG_EINVAL, "jg_tpset_merge_json: mode %u (0 = automatic, 1 = serial parser only)", mode);
        check_offsets("jg_tpset_merge_json", n, off, bytes);
        s->stats = jg_tpset_stats{};
        s->stats.tile_bytes = kTile;
        if (n == 0) return;
        jg_ctx* ctx = s->ctx;
        hipStream_t st = ctx->stream;
        jg::ensure_device(ctx);
        const uint64_t nb = off[n];

        // tiles: message m's run from the 16-byte line its first byte lies in
        std::vector<uint32_t> tile_msg;
        std::vector<ull> tile_at, msg_tile0(n + 1);
        if (mode == 0) {
            for (uint64_t m = 0; m < n; ++m) {
                msg_tile0[m] = tile_msg.size();
                if (off[m] == off[m + 1]) continue;
                for (uint64_t at = off[m] & ~15ull; at < off[m + 1]; at += kTile) tile_msg.push_back((uint32_t)m), tile_at.push_back(at);
            }
            msg_tile0[n] = tile_msg.size();
        }
        const uint64_t T = tile_msg.size();

        uint8_t *d_bytes = nullptr, *d_tmp = nullptr, *d_flat = nullptr, *d_status = nullptr, *d_tstate = nullptr;
        ull *d_off = nullptr, *d_first = nullptr, *d_cbase = nullptr, *d_small = nullptr, *d_tile_at = nullptr, *d_tile0 = nullptr, *d_tbase = nullptr;
        uint32_t *d_cnt = nullptr, *d_tile_msg = nullptr, *d_tfn = nullptr, *d_tcnt = nullptr;
        uint16_t* d_emask = nullptr;
        MsgScan* d_ms = nullptr;
        jg::Layout cv;
        cv.add<uint8_t>(d_bytes, nb + 64), cv.add<uint8_t>(d_tmp, nb + 64), cv.add<ull>(d_off, n + 1);
        cv.add<uint8_t>(d_flat, n), cv.add<uint8_t>(d_status, n), cv.add<uint32_t>(d_cnt, 2 * n), cv.add<ull>(d_first, 2 * n);
        cv.add<ull>(d_cbase, 2 * n + 1), cv.add<ull>(d_small, 8), cv.add<MsgScan>(d_ms, n);
        cv.add<uint32_t>(d_tile_msg, T), cv.add<ull>(d_tile_at, T), cv.add<ull>(d_tile0, n + 1), cv.add<uint32_t>(d_tfn, T);
        cv.add<uint8_t>(d_tstate, T), cv.add<uint32_t>(d_tcnt, T), cv.add<ull>(d_tbase, T + 1), cv.add<uint16_t>(d_emask, T * kBlock);
        cv.bind(work(s, s->w1, cv.bytes() + 1024));
        ull* d_bad = d_small;       // [0] first bad message
        ull* d_stat = d_small + 1;  // [0..1] messages / bytes the scanner took
        ull* d_lim = d_small + 3;   // [0..2] k_limit

        if (nb) JG_HIP(hipMemcpyAsync(d_bytes, bytes, nb, hipMemcpyHostToDevice, st));
        JG_HIP(hipMemsetAsync(d_bytes + nb, 0, 64, st));
        JG_HIP(hipMemcpyAsync(d_off, off, (n + 1) * 8, hipMemcpyHostToDevice, st));
        JG_HIP(hipEventRecord(s->ev0, st));
        JG_HIP(hipMemsetAsync(d_small, 0, 64, st));
        JG_HIP(hipMemsetAsync(d_bad, 0xFF, 8, st));
        JG_HIP(hipMemsetAsync(d_flat, 0, n, st));
        const unsigned gm = blocks_for(n);
        ull* d_epos = nullptr;
        uint32_t* d_emsg = nullptr;
        uint64_t E = 0;
        if (T) {
            JG_HIP(hipMemcpyAsync(d_tile_msg, tile_msg.data(), T * 4, hipMemcpyHostToDevice, st));
            JG_HIP(hipMemcpyAsync(d_tile_at, tile_at.data(), T * 8, hipMemcpyHostToDevice, st));
            JG_HIP(hipMemcpyAsync(d_tile0, msg_tile0.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_msg_init, dim3(gm), dim3(kBlock), 0, st, d_ms, n);
            hipLaunchKernelGGL(k_tile_fn, dim3((unsigned)T), dim3(kBlock), 0, st, d_bytes, d_off, d_tile_msg, d_tile_at, d_tfn);
            hipLaunchKernelGGL(k_tile_carry, dim3(1), dim3(kBlock), 0, st, d_tfn, d_tile_msg, T, d_tstate);
            hipLaunchKernelGGL(k_mark, dim3((unsigned)T), dim3(kBlock), 0, st, d_bytes, d_off, d_tile_msg, d_tile_at, d_tstate, d_ms, d_emask, d_tcnt);
            excl_scan(s, d_tcnt, d_tbase, T);
            JG_HIP(hipGetLastError());
            E = pin_read(ctx, d_tbase + T);
            jg::Layout cv2;
            cv2.add<ull>(d_epos, E + 1), cv2.add<uint32_t>(d_emsg, E + 1);
            cv2.bind(work(s, s->w2, cv2.bytes() + 1024));
            hipLaunchKernelGGL(k_emit, dim3((unsigned)T), dim3(kBlock), 0, st, d_tile_msg, d_tile_at, d_emask, d_tbase, d_epos, d_emsg);
            if (E) hipLaunchKernelGGL(k_strings, dim3(blocks_for(E)), dim3(kBlock), 0, st, d_bytes, d_off, d_epos, d_emsg, E, d_ms);
            hipLaunchKernelGGL(k_walk, dim3(gm), dim3(kBlock), 0, st, d_bytes, d_off, n, d_ms, d_tbase, d_tile0, d_epos, d_flat, d_cnt, d_first, d_stat);
        }
        hipLaunchKernelGGL(k_serial, dim3(gm), dim3(kBlock), 0, st, d_bytes, d_off, n, d_flat, d_status, d_cnt, d_first, d_bad);
        excl_scan(s, d_cnt, d_cbase, 2 * n);
        hipLaunchKernelGGL(k_limit, dim3(1), dim3(1), 0, st, d_bad, d_status, d_cbase, n, d_lim);
        JG_HIP(hipGetLastError());
        jg::pin_get(ctx, 0, d_small, 64);
        jg::pin_sync(ctx);
        uint64_t small[8];
        std::memcpy(small, jg::pin_at(ctx, 0), 64);
        const uint64_t bad = small[3], bad_status = small[4], C = small[5];
        JG_REQUIRE(C < 0xFFFFFFF0ull, JG_EINVAL, "jg_tpset_merge_json: too many strings in one call");
        s->stats.msgs_parallel = small[1], s->stats.bytes_parallel = small[2];
        s->stats.msgs_serial = n - small[1], s->stats.bytes_serial = nb - small[2];
        s->stats.strings_seen = C;

        if (C) {
            CandBufs B{};
            ull* d_cpos = nullptr;
            jg::Layout cv3;
            cv3.add<ull>(d_cpos, C);
            cand_layout(cv3, C, B);
            cv3.bind(work(s, s->w3, cv3.bytes() + 1024));
            B.K.tmp = d_tmp;
            if (E) hipLaunchKernelGGL(k_place, dim3(blocks_for(E)), dim3(kBlock), 0, st, d_epos, d_emsg, E, d_flat, d_cnt, d_first, d_cbase, C, d_cpos, B.K.cwhich);
            hipLaunchKernelGGL(k_serial_emit, dim3(gm), dim3(kBlock), 0, st, d_bytes, d_off, n, d_flat, d_status, d_cnt, d_first, d_cbase, C, d_cpos,
                               B.K.cwhich);
            hipLaunchKernelGGL(k_cand_hash, dim3(blocks_for(C)), dim3(kBlock), 0, st, d_bytes, nb, d_tmp, d_cpos, C, s->salt, B.K.cstart, B.K.clen, B.K.ckey,
                               B.K.cwhich);
            JG_HIP(hipGetLastError());
            s->stats.strings_new = insert_candidates(s, B, false, "jg_tpset_merge_json");
        }
        JG_HIP(hipEventRecord(s->ev1, st));
        JG_HIP(hipEventSynchronize(s->ev1));
        float ms = 0;
        JG_HIP(hipEventElapsedTime(&ms, s->ev0, s->ev1));
        s->stats.device_s = ms * 1e-3;
        if (bad < n) {
            if (bad_msg) *bad_msg = bad;
            if (partial) *partial = bad_status == 2;
            jg::fail(JG_EINVAL, bad_status == 2 ? "jg_tpset_merge_json: message %llu has no removeSet: its addSet was merged, nothing after it"
                                                : "jg_tpset_merge_json: message %llu is not a TPSetMsg in the accepted form: nothing from it on was merged",
                     (ull)bad);
        }
    });
}

int jg_tpset_encode_json(jg_tpset* s, uint64_t* n_bytes, uint8_t* out, uint64_t cap) {
    return jg::guard([&] {
        auto lk_ = jg::lock(s);
        JG_REQUIRE(s && n_bytes, JG_EINVAL, "jg_tpset_encode_json: NULL argument");
        jg_ctx* ctx = s->ctx;
        hipStream_t st = ctx->stream;
        jg::ensure_device(ctx);
        const uint64_t ne = s->n_add + s->n_rem;
        static const char kEmpty[] = "{\"addSet\":[],\"removeSet\":[]}";
        if (ne == 0) {  // no entry owns a piece: the empty message is a constant
            *n_bytes = sizeof kEmpty - 1;
            if (!out) return;
            JG_REQUIRE(*n_bytes <= cap, JG_ESTATE, "jg_tpset_encode_json: %llu bytes exceed the buffer's %llu", (ull)*n_bytes, (ull)cap);
            std::memcpy(out, kEmpty, sizeof kEmpty - 1);
            return;
        }
        uint32_t* len = nullptr;
        ull* eo = nullptr;
        jg::Layout cv;
        cv.add<uint32_t>(len, ne + 1), cv.add<ull>(eo, ne + 2);
        cv.bind(work(s, s->w3, cv.bytes() + 1024));
        const Store S = s->view();
        JG_HIP(hipEventRecord(s->ev0, st));
        hipLaunchKernelGGL(k_enc_len, dim3(blocks_for(ne)), dim3(kBlock), 0, st, S, s->n_add, s->n_rem, len);
        excl_scan(s, len, eo, ne);
        JG_HIP(hipGetLastError());
        const uint64_t total = pin_read(ctx, eo + ne);
        *n_bytes = total;
        if (!out) return;
        JG_REQUIRE(total <= cap, JG_ESTATE, "jg_tpset_encode_json: %llu bytes exceed the buffer's %llu", (ull)total, (ull)cap);
        uint8_t* d_out = static_cast<uint8_t*>(work(s, s->w2, total + 64));
        hipLaunchKernelGGL(k_enc_write, dim3(blocks_for(ne)), dim3(kBlock), 0, st, S, s->n_add, s->n_rem, eo, d_out);
        JG_HIP(hipGetLastError());
        JG_HIP(hipEventRecord(s->ev1, st));
        JG_HIP(hipMemcpyAsync(out, d_out, total, hipMemcpyDeviceToHost, st));
        JG_HIP(hipStreamSynchronize(st));
        float ms = 0;
        JG_HIP(hipEventElapsedTime(&ms, s->ev0, s->ev1));
        s->encode_s = ms * 1e-3;
    });
}

int jg_tpset_last_stats(jg_tpset* s, jg_tpset_stats* out) {
    return jg::guard([&] {
        auto lk_ = jg::lock(s);
        JG_REQUIRE(s && out, JG_EINVAL, "jg_tpset_last_stats: NULL argument");
        *out = s->stats;
        out->tile_bytes = kTile;
        out->stage_bytes = kStage;
        out->encode_s = s->encode_s;
    });
}

}  // extern "C"

// =====================================================================================================
// jg_keyspace — KeySpaceManager's state (BFT-CRDT/CRDTManagers/KeySpaceManager.cs): the set, the keySpaces dictionary
// and the LastKeySpaceSet watermark.  Every entry is key + "\0" + guid in the set's pool, so a dictionary entry holds
// no bytes of its own: (string id of the entry that introduced the key, key length, guid).  Nothing leaves either
// HashSet, so "LookupAll().Except(LastKeySpaceSet)" (:157-159) is the present entries from the add ordinal the last
// OnNext ended at.
// =====================================================================================================
namespace {

struct Items {  // one dictionary candidate per item, in order; klen = the key's bytes, rlen = the bytes its journal record copies
    uint32_t *sid, *klen, *rlen, *slot, *prep, *pmin;
    ull *glo, *ghi, *key;
    uint8_t *status, *valid;
    uint64_t pmask, n;
};

// OnNext's body per new entry (KeySpaceManager.cs:160-172), entry = add[from + i]: seen iff not in removeSet; key =
// the bytes before the first NUL (the whole entry if it has none), guid = the segment up to the second NUL in "D" form.
// status is what jg_keyspace_new_keys reports if the key turns out unknown (k_ks_find / k_ks_win decide that); a
// malformed entry carries its key's hash and length as well, since ContainsKey (:164) comes before Guid.Parse (:166).
__global__ void k_ks_parse(Store S, uint64_t from, Items I) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= I.n) return;
    const uint32_t id = S.add[from + i];
    I.sid[i] = id, I.slot[i] = kNone, I.glo[i] = I.ghi[i] = 0, I.key[i] = 0;
    if (id == kNullId) {
        I.valid[i] = S.nulls[1] == kNone, I.status[i] = 3, I.klen[i] = I.rlen[i] = 0;
        return;
    }
    I.valid[i] = S.srem[id] == kNone;
    const uint8_t* s = S.pool + S.soff[id];
    const uint32_t len = S.slen[id];
    uint32_t p1 = 0;
    while (p1 < len && s[p1]) ++p1;
    I.klen[i] = p1, I.rlen[i] = len, I.key[i] = key_hash(s, p1, S.salt);
    if (p1 == len) {
        I.status[i] = 1;
        return;
    }
    jgw::GuidSink g;
    for (uint32_t p = p1 + 1; p < len && s[p]; ++p) g.put(s[p]);
    if (!g.ok()) {
        I.status[i] = 2;
        return;
    }
    I.status[i] = 0, I.rlen[i] = p1, I.glo[i] = g.lo(), I.ghi[i] = g.hi;
}

// CreateNewKVPair's TryAdd (:130): item i = key i of the batch, found as the prefix of its entry in the set
__global__ void k_ks_local(Store S, const uint8_t* __restrict__ ent, const ull* __restrict__ eoff, const uint32_t* __restrict__ klen,
                           const jg_guid* __restrict__ guid, Items I) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= I.n) return;
    const uint8_t* e = ent + eoff[i];
    const uint32_t len = (uint32_t)(eoff[i + 1] - eoff[i]);
    I.sid[i] = store_find(S, key_hash(e, len, S.salt), e, len);  // the Add before this launch put it there
    I.klen[i] = I.rlen[i] = klen[i], I.slot[i] = kNone, I.glo[i] = guid[i].lo, I.ghi[i] = guid[i].hi;
    I.key[i] = key_hash(e, klen[i], S.salt);
    I.status[i] = 0, I.valid[i] = 1;
}

// first wins: among the well-formed items whose key the dictionary lacks, the smallest index per distinct key
__global__ void k_ks_find(Store S, Dict D, Items I) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= I.n || !I.valid[i] || I.status[i]) return;
    const uint8_t* k = S.pool + S.soff[I.sid[i]];
    const uint32_t klen = I.klen[i];
    if (dict_find(S, D, I.key[i], k, klen) != kNone) return;
    for (uint64_t slot = I.key[i] & I.pmask;; slot = (slot + 1) & I.pmask) {
        uint32_t r = I.prep[slot];
        if (r == 0) {
            r = atomicCAS(&I.prep[slot], 0u, (uint32_t)i + 1);
            if (r == 0) r = (uint32_t)i + 1;
        }
        const uint32_t o = r - 1;
        if (I.key[o] == I.key[i] && I.klen[o] == klen && same_bytes(S.pool + S.soff[I.sid[o]], k, klen)) {
            atomicMin(&I.pmin[slot], (uint32_t)i);
            I.slot[i] = (uint32_t)slot;
            return;
        }
    }
}
// added = the item puts its key into the dictionary; jrn = it is journalled: an added key, the null element, or a
// malformed entry whose key is unknown when its turn comes, i.e. neither in the dictionary nor added by a well-formed
// item before it (the minima stand: k_ks_find has ended, the call-wide table is only read here)
__global__ void k_ks_win(Store S, Dict D, Items I, uint32_t* __restrict__ added, uint32_t* __restrict__ jrn) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= I.n) return;
    const bool a = I.slot[i] != kNone && I.pmin[I.slot[i]] == i;
    added[i] = a;
    bool j = a;
    if (I.valid[i] && I.status[i] == 3) j = true;
    else if (I.valid[i] && I.status[i] != 0) {
        const uint8_t* k = S.pool + S.soff[I.sid[i]];
        const uint32_t klen = I.klen[i];
        j = dict_find(S, D, I.key[i], k, klen) == kNone;
        for (uint64_t slot = I.key[i] & I.pmask; j; slot = (slot + 1) & I.pmask) {
            const uint32_t r = I.prep[slot];
            if (r == 0) break;
            const uint32_t o = r - 1;
            if (I.key[o] == I.key[i] && I.klen[o] == klen && same_bytes(S.pool + S.soff[I.sid[o]], k, klen)) {
                j = I.pmin[slot] > i;
                break;
            }
        }
    }
    jrn[i] = j;
}
__global__ void k_ks_commit(Dict D, Items I, const uint32_t* __restrict__ added, const ull* __restrict__ oa, uint64_t n_keys, const uint32_t* __restrict__ jrn,
                            const ull* __restrict__ oj, uint64_t jn, uint32_t* __restrict__ jsid, uint32_t* __restrict__ jlen, ull* __restrict__ jglo,
                            ull* __restrict__ jghi, uint8_t* __restrict__ jstatus) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= I.n) return;
    if (added[i]) {
        const uint32_t d = (uint32_t)(n_keys + oa[i]);
        D.sid[d] = I.sid[i], D.klen[d] = I.klen[i], D.glo[d] = I.glo[i], D.ghi[d] = I.ghi[i], D.key[d] = I.key[i];
        for (uint64_t slot = I.key[i] & D.mask;; slot = (slot + 1) & D.mask)
            if (D.table[slot] == 0 && atomicCAS(&D.table[slot], 0u, d + 1) == 0) break;
    }
    if (jsid && jrn[i]) {
        const ull j = jn + oj[i];
        jsid[j] = I.sid[i], jlen[j] = I.rlen[i], jglo[j] = I.glo[i], jghi[j] = I.ghi[i], jstatus[j] = I.status[i];
    }
}

__global__ void k_ks_lookup(Store S, Dict D, const uint8_t* __restrict__ keys, const ull* __restrict__ off, uint64_t n, jg_guid* __restrict__ guid,
                            uint8_t* __restrict__ found) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t* k = keys + off[i];
    const uint32_t klen = (uint32_t)(off[i + 1] - off[i]);
    const uint32_t d = dict_find(S, D, key_hash(k, klen, S.salt), k, klen);
    found[i] = d != kNone;
    guid[i] = d != kNone ? jg_guid{D.glo[d], D.ghi[d]} : jg_guid{0, 0};
}

__global__ void k_ks_journal(Store S, uint64_t from, uint64_t n, const uint32_t* __restrict__ jsid, const uint32_t* __restrict__ jlen,
                             const ull* __restrict__ jglo, const ull* __restrict__ jghi, const uint8_t* __restrict__ jstatus, const ull* __restrict__ ob,
                             ull* __restrict__ off, uint8_t* __restrict__ bytes, jg_guid* __restrict__ guid, uint8_t* __restrict__ status) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) off[n] = ob[n];
    if (i >= n) return;
    const uint64_t j = from + i;
    off[i] = ob[i], guid[i] = jg_guid{jglo[j], jghi[j]}, status[i] = jstatus[j];
    if (jsid[j] == kNullId) return;
    const uint8_t* s = S.pool + S.soff[jsid[j]];
    for (uint32_t k = 0; k < jlen[j]; ++k) bytes[ob[i] + k] = s[k];
}

struct ItemBufs {
    Items I;
    uint32_t *added, *jrn;
    ull *oa, *oj;
};
void items_layout(jg::Layout& cv, uint64_t n, ItemBufs& B) {
    uint64_t slots = 64;
    while (slots < 2 * n) slots <<= 1;
    Items& I = B.I;
    cv.add<uint32_t>(I.sid, n), cv.add<uint32_t>(I.klen, n), cv.add<uint32_t>(I.rlen, n), cv.add<uint32_t>(I.slot, n), cv.add<uint32_t>(I.prep, slots), cv.add<uint32_t>(I.pmin, slots);
    cv.add<ull>(I.glo, n), cv.add<ull>(I.ghi, n), cv.add<ull>(I.key, n), cv.add<uint8_t>(I.status, n), cv.add<uint8_t>(I.valid, n);
    I.pmask = slots - 1, I.n = n;
    cv.add<uint32_t>(B.added, n), cv.add<uint32_t>(B.jrn, n), cv.add<ull>(B.oa, n + 1), cv.add<ull>(B.oj, n + 1);
}
// the items are filled: resolve them against the dictionary in order, append the journal (journal = false: none).
// Returns the journal records appended; added_out (host, optional) = each item's TryAdd bool.
uint64_t dict_insert(jg_keyspace* ks, ItemBufs& B, bool journal, uint8_t* added_out) {
    jg_tpset* s = ks->set;
    hipStream_t st = ks->ctx->stream;
    const uint64_t n = B.I.n, slots = B.I.pmask + 1;
    const unsigned g = blocks_for(n);
    JG_HIP(hipMemsetAsync(B.I.prep, 0, slots * 4, st));
    JG_HIP(hipMemsetAsync(B.I.pmin, 0xFF, slots * 4, st));
    hipLaunchKernelGGL(k_ks_find, dim3(g), dim3(kBlock), 0, st, s->view(), ks->dict(), B.I);
    hipLaunchKernelGGL(k_ks_win, dim3(g), dim3(kBlock), 0, st, s->view(), ks->dict(), B.I, B.added, B.jrn);
    excl_scan(s, B.added, B.oa, n);
    excl_scan(s, B.jrn, B.oj, n);
    JG_HIP(hipGetLastError());
    jg::pin_get(ks->ctx, 0, B.oa + n, 8);
    jg::pin_get(ks->ctx, 8, B.oj + n, 8);
    jg::pin_sync(ks->ctx);
    const uint64_t ta = static_cast<const uint64_t*>(jg::pin_at(ks->ctx, 0))[0], tj = static_cast<const uint64_t*>(jg::pin_at(ks->ctx, 0))[1];
    JG_REQUIRE(ks->n_keys + ta <= ks->cap + 1 && ks->jn + tj <= ks->cap + 1, JG_ESTATE, "jg_keyspace: dictionary or journal full");
    hipLaunchKernelGGL(k_ks_commit, dim3(g), dim3(kBlock), 0, st, ks->dict(), B.I, B.added, B.oa, ks->n_keys, B.jrn, B.oj, ks->jn,
                       journal ? ks->jsid.as<uint32_t>() : (uint32_t*)nullptr, ks->jlen.as<uint32_t>(), ks->jglo.as<ull>(), ks->jghi.as<ull>(),
                       ks->jstatus.as<uint8_t>());
    JG_HIP(hipGetLastError());
    if (added_out) {
        std::vector<uint32_t> a(n);
        JG_HIP(hipMemcpyAsync(a.data(), B.added, n * 4, hipMemcpyDeviceToHost, st));
        JG_HIP(hipStreamSynchronize(st));
        for (uint64_t i = 0; i < n; ++i) added_out[i] = (uint8_t)a[i];
    }
    ks->n_keys += ta;
    if (journal) ks->jn += tj;
    return journal ? tj : 0;
}

// KeySpaceManager.OnNext (:151-178) after a merge: the entries from the watermark on
uint64_t on_next(jg_keyspace* ks) {
    jg_tpset* s = ks->set;
    const uint64_t n = s->n_add - ks->seen;
    if (n == 0) return 0;
    ItemBufs B{};
    jg::Layout cv;
    items_layout(cv, n, B);
    cv.bind(work(s, ks->wk, cv.bytes() + 1024));
    hipLaunchKernelGGL(k_ks_parse, dim3(blocks_for(n)), dim3(kBlock), 0, ks->ctx->stream, s->view(), ks->seen, B.I);
    const uint64_t tj = dict_insert(ks, B, true, nullptr);
    ks->seen = s->n_add;
    return tj;
}

void guid_d(const jg_guid& g, char* o) {  // Guid.ToString(): "D", lower case (oracle/json.hpp GuidD)
    static const char* hx = "0123456789abcdef";
    static const int order[16] = {3, 2, 1, 0, 5, 4, 7, 6, 8, 9, 10, 11, 12, 13, 14, 15};
    uint8_t b[16];
    for (int i = 0; i < 8; ++i) b[i] = (uint8_t)(g.lo >> (8 * i)), b[8 + i] = (uint8_t)(g.hi >> (8 * i));
    for (int i = 0; i < 16; ++i) {
        if (i == 4 || i == 6 || i == 8 || i == 10) *o++ = '-';
        *o++ = hx[b[order[i]] >> 4], *o++ = hx[b[order[i]] & 15];
    }
}

}  // namespace

extern "C" {

int jg_keyspace_create(jg_ctx* ctx, uint64_t cap_keys, uint64_t cap_bytes, jg_keyspace** out) {
    return jg::guard([&] {
        JG_REQUIRE(ctx && out, JG_EINVAL, "jg_keyspace_create: NULL argument");
        std::unique_ptr<jg_keyspace> ks(new jg_keyspace());
        ks->ctx = ctx;
        int rc = jg_tpset_create(ctx, cap_keys, cap_bytes, &ks->set);
        if (rc != JG_OK) {
            char buf[512];
            jg_last_error(buf, sizeof buf);
            jg::fail(rc, "%s", buf);
        }
        auto lk_ = jg::lock(ctx);
        ks->cap = cap_keys;
        uint64_t slots = 64;
        while (slots < 2 * (cap_keys + 2)) slots <<= 1;
        ks->mask = slots - 1;
        const uint64_t n = cap_keys + 2;
        ks->table.alloc(slots * 4), ks->dsid.alloc(n * 4), ks->dklen.alloc(n * 4), ks->dglo.alloc(n * 8), ks->dghi.alloc(n * 8), ks->dkey.alloc(n * 8);
        ks->jsid.alloc(n * 4), ks->jlen.alloc(n * 4), ks->jglo.alloc(n * 8), ks->jghi.alloc(n * 8), ks->jstatus.alloc(n);
        JG_HIP(hipMemsetAsync(ks->table.p, 0, slots * 4, ctx->stream));
        JG_HIP(hipStreamSynchronize(ctx->stream));
        *out = ks.release();
    });
}

int jg_keyspace_destroy(jg_keyspace* ks) {
    if (!ks) return JG_OK;
    const int rc = jg_tpset_destroy(ks->set);
    delete ks;
    return rc;
}

int jg_keyspace_set(jg_keyspace* ks, jg_tpset** set) {
    return jg::guard([&] {
        JG_REQUIRE(ks && set, JG_EINVAL, "jg_keyspace_set: NULL argument");
        *set = ks->set;
    });
}

int jg_keyspace_create_keys(jg_keyspace* ks, uint64_t n, const uint64_t* off, const uint8_t* key_bytes, const jg_guid* guid, uint8_t* added) {
    return jg::guard([&] {
        auto lk_ = jg::lock(ks);
        JG_REQUIRE(ks && (n == 0 || guid), JG_EINVAL, "jg_keyspace_create_keys: NULL argument");
        check_offsets("jg_keyspace_create_keys", n, off, key_bytes);
        if (n == 0) return;
        // Add(key + "\0" + guid.ToString()) regardless of the TryAdd (:130-131)
        std::vector<uint64_t> eoff(n + 1, 0);
        std::vector<uint32_t> klen(n);
        std::vector<uint8_t> ent, op(n, 1);
        for (uint64_t i = 0; i < n; ++i) {
            klen[i] = (uint32_t)(off[i + 1] - off[i]);
            ent.insert(ent.end(), key_bytes + off[i], key_bytes + off[i + 1]);
            ent.push_back(0);
            char g[36];
            guid_d(guid[i], g);
            ent.insert(ent.end(), g, g + 36);
            eoff[i + 1] = ent.size();
        }
        const int rc = jg_tpset_apply_ops(ks->set, n, op.data(), eoff.data(), ent.data(), nullptr, nullptr);
        if (rc != JG_OK) {
            char buf[512];
            jg_last_error(buf, sizeof buf);
            jg::fail(rc, "%s", buf);
        }
        jg_tpset* s = ks->set;
        hipStream_t st = ks->ctx->stream;
        jg::ensure_device(ks->ctx);
        ItemBufs B{};
        uint8_t* d_ent = nullptr;
        ull* d_eoff = nullptr;
        uint32_t* d_klen = nullptr;
        jg_guid* d_guid = nullptr;
        jg::Layout cv;
        cv.add<uint8_t>(d_ent, ent.size() + 16), cv.add<ull>(d_eoff, n + 1), cv.add<uint32_t>(d_klen, n), cv.add<jg_guid>(d_guid, n);
        items_layout(cv, n, B);
        cv.bind(work(s, ks->wk, cv.bytes() + 1024));
        JG_HIP(hipMemcpyAsync(d_ent, ent.data(), ent.size(), hipMemcpyHostToDevice, st));
        JG_HIP(hipMemcpyAsync(d_eoff, eoff.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
        JG_HIP(hipMemcpyAsync(d_klen, klen.data(), n * 4, hipMemcpyHostToDevice, st));
        JG_HIP(hipMemcpyAsync(d_guid, guid, n * sizeof(jg_guid), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_ks_local, dim3(blocks_for(n)), dim3(kBlock), 0, st, s->view(), d_ent, d_eoff, d_klen, d_guid, B.I);
        std::vector<uint8_t> tmp(n);
        dict_insert(ks, B, false, added ? added : tmp.data());
    });
}

int jg_keyspace_receive(jg_keyspace* ks, uint64_t n, const uint64_t* off, const uint8_t* bytes, uint32_t mode, uint64_t* bad_msg, uint8_t* partial,
                        uint64_t* n_new) {
    if (bad_msg) *bad_msg = UINT64_MAX;
    if (partial) *partial = 0;
    if (n_new) *n_new = 0;
    return jg::guard([&] {
        auto lk_ = jg::lock(ks);
        JG_REQUIRE(ks, JG_EINVAL, "jg_keyspace_receive: keyspace is NULL");
        check_offsets("jg_keyspace_receive", n, off, bytes);
        jg::ensure_device(ks->ctx);
        uint64_t total = 0;
        // message after message: Merge, then OnNext over what it left present (a later message's removal cannot
        // unsee an entry, and an entry its own message also removes is never seen)
        for (uint64_t m = 0; m < n; ++m) {
            const uint64_t o[2] = {0, off[m + 1] - off[m]};
            uint64_t bad;
            uint8_t part;
            const int rc = jg_tpset_merge_json(ks->set, 1, o, bytes + off[m], mode, &bad, &part);
            if (rc != JG_OK) {  // the reference's Decode / Merge throws before OnNext: the watermark stays
                if (bad_msg && rc == JG_EINVAL) *bad_msg = m;
                if (partial) *partial = part;
                if (n_new) *n_new = total;
                char buf[512];
                jg_last_error(buf, sizeof buf);
                jg::fail(rc, "jg_keyspace_receive: message %llu: %s", (ull)m, buf);
            }
            total += on_next(ks);
        }
        if (n_new) *n_new = total;
    });
}

int jg_keyspace_new_keys(jg_keyspace* ks, uint64_t from, uint64_t* to, uint64_t* n_bytes, uint64_t* off, uint8_t* bytes, jg_guid* guid, uint8_t* status) {
    return jg::guard([&] {
        auto lk_ = jg::lock(ks);
        JG_REQUIRE(ks && to && n_bytes, JG_EINVAL, "jg_keyspace_new_keys: NULL argument");
        JG_REQUIRE(from <= ks->jn, JG_EINVAL, "jg_keyspace_new_keys: from %llu past the journal's %llu", (ull)from, (ull)ks->jn);
        const bool query = !off && !bytes && !guid && !status;
        JG_REQUIRE(query || (off && guid && status), JG_EINVAL, "jg_keyspace_new_keys: off, guid, status: all or none");
        jg_tpset* s = ks->set;
        hipStream_t st = ks->ctx->stream;
        jg::ensure_device(ks->ctx);
        const uint64_t n = ks->jn - from, cap_b = *n_bytes;
        *to = ks->jn;
        if (n == 0) {
            *n_bytes = 0;
            if (off) off[0] = 0;
            return;
        }
        ull *ob = nullptr, *d_off = nullptr;
        uint8_t *d_bytes = nullptr, *d_status = nullptr;
        jg_guid* d_guid = nullptr;
        jg::Layout cv;
        cv.add<ull>(ob, n + 1), cv.add<ull>(d_off, n + 1), cv.add<jg_guid>(d_guid, n), cv.add<uint8_t>(d_status, n);
        cv.add<uint8_t>(d_bytes, s->n_bytes + 16);
        cv.bind(work(s, ks->wk, cv.bytes() + 1024));
        excl_scan(s, ks->jlen.as<uint32_t>() + from, ob, n);
        if (!query)
            hipLaunchKernelGGL(k_ks_journal, dim3(blocks_for(n)), dim3(kBlock), 0, st, s->view(), from, n, ks->jsid.as<uint32_t>(), ks->jlen.as<uint32_t>(),
                               ks->jglo.as<ull>(), ks->jghi.as<ull>(), ks->jstatus.as<uint8_t>(), ob, d_off, d_bytes, d_guid, d_status);
        JG_HIP(hipGetLastError());
        const uint64_t nb = pin_read(ks->ctx, ob + n);
        *n_bytes = nb;
        if (query) return;
        JG_REQUIRE(nb <= cap_b && (nb == 0 || bytes), JG_ESTATE, "jg_keyspace_new_keys: %llu bytes exceed the buffer", (ull)nb);
        JG_HIP(hipMemcpyAsync(off, d_off, (n + 1) * 8, hipMemcpyDeviceToHost, st));
        JG_HIP(hipMemcpyAsync(guid, d_guid, n * sizeof(jg_guid), hipMemcpyDeviceToHost, st));
        JG_HIP(hipMemcpyAsync(status, d_status, n, hipMemcpyDeviceToHost, st));
        if (nb) JG_HIP(hipMemcpyAsync(bytes, d_bytes, nb, hipMemcpyDeviceToHost, st));
        JG_HIP(hipStreamSynchronize(st));
    });
}

int jg_keyspace_lookup(jg_keyspace* ks, uint64_t n, const uint64_t* off, const uint8_t* key_bytes, jg_guid* guid, uint8_t* found) {
    return jg::guard([&] {
        auto lk_ = jg::lock(ks);
        JG_REQUIRE(ks && (n == 0 || (guid && found)), JG_EINVAL, "jg_keyspace_lookup: NULL argument");
        check_offsets("jg_keyspace_lookup", n, off, key_bytes);
        if (n == 0) return;
        jg_tpset* s = ks->set;
        hipStream_t st = ks->ctx->stream;
        jg::ensure_device(ks->ctx);
        uint8_t *d_keys = nullptr, *d_found = nullptr;
        ull* d_off = nullptr;
        jg_guid* d_guid = nullptr;
        jg::Layout cv;
        cv.add<uint8_t>(d_keys, off[n] + 16), cv.add<ull>(d_off, n + 1), cv.add<jg_guid>(d_guid, n), cv.add<uint8_t>(d_found, n);
        cv.bind(work(s, ks->wk, cv.bytes() + 1024));
        if (off[n]) JG_HIP(hipMemcpyAsync(d_keys, key_bytes, off[n], hipMemcpyHostToDevice, st));
        JG_HIP(hipMemcpyAsync(d_off, off, (n + 1) * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_ks_lookup, dim3(blocks_for(n)), dim3(kBlock), 0, st, s->view(), ks->dict(), d_keys, d_off, n, d_guid, d_found);
        JG_HIP(hipGetLastError());
        JG_HIP(hipMemcpyAsync(guid, d_guid, n * sizeof(jg_guid), hipMemcpyDeviceToHost, st));
        JG_HIP(hipMemcpyAsync(found, d_found, n, hipMemcpyDeviceToHost, st));
        JG_HIP(hipStreamSynchronize(st));
    });
}

}  // extern "C"
