// tpset_encode.hip — jg_tpset_encode_json: TPSetMsg.Encode() (MergeSharp/MergeSharp/CRDTs/2P-Set.cs:49-52) of the
// whole resident set.  Owns the escaping rule, the pieces of the wire form and the two passes over them:
//   k_enc_len -> count scan of the pieces' lengths -> (the total read back) -> k_enc_write
// It only reads the store (tpset_dict.hpp); the set itself is tpset.hip's.  DESIGN.md §Key-space set.
#include <cstring>

#include "tpset_host.hpp"

using namespace jgt;

namespace {

using jg::blocks_for;

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

}  // namespace

uint32_t jgt::encode_stage_bytes() { return kStage; }

extern "C" int jg_tpset_encode_json(jg_tpset* s, uint64_t* n_bytes, uint8_t* out, uint64_t cap) {
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
        cv.bind(work(ctx, s->w3, cv.bytes() + 1024));
        const Store S = s->view();
        JG_HIP(hipEventRecord(s->ev0, st));
        hipLaunchKernelGGL(k_enc_len, dim3(blocks_for(ne)), dim3(kBlock), 0, st, S, s->n_add, s->n_rem, len);
        excl_scan(ctx, s->wscan, len, eo, ne);
        JG_HIP(hipGetLastError());
        const uint64_t total = read_totals(ctx, eo + ne)[0];
        *n_bytes = total;
        if (!out) return;
        JG_REQUIRE(total <= cap, JG_ESTATE, "jg_tpset_encode_json: %llu bytes exceed the buffer's %llu", (ull)total, (ull)cap);
        uint8_t* d_out = static_cast<uint8_t*>(work(ctx, s->w2, total + 64));
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
