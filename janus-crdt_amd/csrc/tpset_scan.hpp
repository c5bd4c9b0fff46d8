// tpset_scan.hpp — the parallel scanner of a call's TPSetMsg payloads: which messages are flat (one addSet array, one
// removeSet array, nothing else), and where every element of a flat message starts.  Device-only; tpset.hip launches
//   k_msg_init, k_tile_fn -> k_tile_carry -> k_mark -> (count scan) -> k_emit -> k_strings -> k_walk
// and hands every message k_walk did not prove flat to the serial parser of tpset_wire.hpp, the form's definition.
#pragma once

#include "block_scan.hpp"
#include "tpset_wire.hpp"

namespace {

using jgt::kNone;
using jgt::umin;

constexpr uint32_t kTile = kBlock * 16;  // bytes of one scanner tile: 16 B per lane

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
    block_scan_incl<kBlock>(f, sh, [](uint32_t a, uint32_t b) { return fn_then(a, b); });
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

// element g of the call = the position of its first byte, in text order
__global__ __launch_bounds__(kBlock) void k_emit(const uint32_t* __restrict__ tile_msg, const ull* __restrict__ tile_at, const uint16_t* __restrict__ emask,
                                                 const ull* __restrict__ tbase, ull* __restrict__ epos, uint32_t* __restrict__ emsg) {
    __shared__ uint32_t sh[kBlock];
    const uint32_t tile = blockIdx.x, t = threadIdx.x;
    uint32_t mask = emask[(uint64_t)tile * kBlock + t];
    block_scan_incl<kBlock>((uint32_t)__popc(mask), sh, ScanAdd{});
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

}  // namespace
