// tpset.hip — one TPSet<string?> resident on the device (MergeSharp/MergeSharp/CRDTs/2P-Set.cs): the replicated
// key-space set of BFT-CRDT/CRDTManagers/KeySpaceManager.cs:34,87.  DESIGN.md §Key-space set.
//
// Owns the resident set: its candidates, their insertion, the queries, and every jg_tpset_* entry point but the encoder
// (tpset_encode.hip).  The wire form is tpset_wire.hpp's, the scanner tpset_scan.hpp's, the count scan block_scan.hpp's
// (launched from here: jgt::excl_scan); the key space over this set is keyspace.hip.
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

#include "tpset_host.hpp"
#include "tpset_scan.hpp"

using namespace jgt;  // the store / dictionary views and their probes (shared with query.hip)

namespace {

using jg::blocks_for;

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

// slot of candidate c's string in the call-wide table (claimed for c if no candidate holds the string yet)
__device__ uint32_t cand_slot(const Cands& K, uint64_t c) {
    const uint8_t* s = K.tmp + K.cstart[c];
    const uint32_t len = K.clen[c];
    const ull key = K.ckey[c];
    return claim_slot(K.prep, K.pmask, key, (uint32_t)c,
                      [&](uint32_t o) { return K.ckey[o] == key && K.clen[o] == len && same_bytes(K.tmp + K.cstart[o], s, len); });
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
// The bytes of a new string come from the slot's representative, the candidate that won claim_slot's CAS, which need
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
    const uint64_t slots = jg::pow2_at_least(2 * C, 64);
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
    excl_scan(ctx, s->wscan, B.wa, B.oa, C);
    excl_scan(ctx, s->wscan, B.wr, B.orr, C);
    excl_scan(ctx, s->wscan, B.ws, B.os, C);
    excl_scan(ctx, s->wscan, B.wb, B.ob, C);
    JG_HIP(hipGetLastError());
    const auto [ta, tr, ts, tb] = read_totals(ctx, B.oa + C, B.orr + C, B.os + C, B.ob + C);
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
    cv.bind(work(ctx, s->w3, cv.bytes() + 1024));
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

// ---- what the units share on the host (tpset_host.hpp) -------------------------------------------------
void* jgt::work(jg_ctx* ctx, jg::DevBuf& b, size_t bytes) {
    if (b.bytes < bytes) {
        JG_HIP(hipStreamSynchronize(ctx->stream));
        b.alloc(bytes + bytes / 4 + 4096);
    }
    return b.p;
}

void jgt::excl_scan(jg_ctx* ctx, jg::DevBuf& block_sums, const uint32_t* in, ull* out, uint64_t n) {
    hipStream_t st = ctx->stream;
    if (n <= 4 * kScanTile) {
        hipLaunchKernelGGL(k_excl_scan<uint32_t>, dim3(1), dim3(1024), 0, st, in, out, n);
        return;
    }
    const uint64_t nb = (n + kScanTile - 1) / kScanTile;
    ull* bsum = static_cast<ull*>(work(ctx, block_sums, (2 * nb + 2) * sizeof(ull)));
    ull* bbase = bsum + nb;
    hipLaunchKernelGGL(k_scan_sum, dim3((unsigned)nb), dim3(kBlock), 0, st, in, n, bsum);
    hipLaunchKernelGGL(k_excl_scan<ull>, dim3(1), dim3(1024), 0, st, (const ull*)bsum, bbase, nb);
    hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)nb), dim3(kBlock), 0, st, in, n, (const ull*)bbase, out);
}

void jgt::check_offsets(const char* fn, uint64_t n, const uint64_t* off, const uint8_t* bytes) {
    JG_REQUIRE(n == 0 || off, JG_EINVAL, "%s: off is NULL", fn);
    if (n == 0) return;
    JG_REQUIRE(off[0] == 0, JG_EINVAL, "%s: off[0] must be 0", fn);
    for (uint64_t i = 0; i < n; ++i) JG_REQUIRE(off[i] <= off[i + 1], JG_EINVAL, "%s: offsets decrease at %llu", fn, (ull)i);
    JG_REQUIRE(off[n] == 0 || bytes, JG_EINVAL, "%s: bytes is NULL", fn);
    JG_REQUIRE(n < 0xFFFFFFF0ull && off[n] < (1ull << 40), JG_EINVAL, "%s: batch too large", fn);
}

jg_tpset* jgt::tpset_create(jg_ctx* ctx, uint64_t cap_strings, uint64_t cap_bytes) {
    JG_REQUIRE(cap_strings < 0x7FFFFFF0ull && cap_bytes < (1ull << 40), JG_EINVAL, "jg_tpset_create: capacity too large");
    jg::ensure_device(ctx);
    std::unique_ptr<jg_tpset> s(new jg_tpset());
    s->ctx = ctx;
    s->cap_strings = cap_strings, s->cap_bytes = cap_bytes;
    const uint64_t slots = jg::pow2_at_least(2 * cap_strings, 64);
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
    return s.release();
}

void jgt::tpset_apply_ops(jg_tpset* s, uint64_t n, const uint8_t* op, const uint64_t* off, const uint8_t* bytes, const uint8_t* is_null, uint8_t* result) {
    JG_REQUIRE(s && (n == 0 || op), JG_EINVAL, "jg_tpset_apply_ops: NULL argument");
    for (uint64_t i = 0; i < n; ++i) JG_REQUIRE(op[i] == 1 || op[i] == 2, JG_EINVAL, "jg_tpset_apply_ops: op %llu has id %u", (ull)i, op[i]);
    if (n == 0) return;
    jg::ensure_device(s->ctx);
    CandBufs B{};
    raw_candidates(s, "jg_tpset_apply_ops", n, op, off, bytes, is_null, B);
    insert_candidates(s, B, true, "jg_tpset_apply_ops");
    if (result) JG_HIP(hipMemcpyAsync(result, B.result, n, hipMemcpyDeviceToHost, s->ctx->stream));
    JG_HIP(hipStreamSynchronize(s->ctx->stream));
}

void jgt::tpset_merge_json(jg_tpset* s, uint64_t n, const uint64_t* off, const uint8_t* bytes, uint32_t mode, uint64_t* bad_msg, uint8_t* partial) {
    if (bad_msg) *bad_msg = UINT64_MAX;
    if (partial) *partial = 0;
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
    cv.bind(work(ctx, s->w1, cv.bytes() + 1024));
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
        excl_scan(ctx, s->wscan, d_tcnt, d_tbase, T);
        JG_HIP(hipGetLastError());
        E = read_totals(ctx, d_tbase + T)[0];
        jg::Layout cv2;
        cv2.add<ull>(d_epos, E + 1), cv2.add<uint32_t>(d_emsg, E + 1);
        cv2.bind(work(ctx, s->w2, cv2.bytes() + 1024));
        hipLaunchKernelGGL(k_emit, dim3((unsigned)T), dim3(kBlock), 0, st, d_tile_msg, d_tile_at, d_emask, d_tbase, d_epos, d_emsg);
        if (E) hipLaunchKernelGGL(k_strings, dim3(blocks_for(E)), dim3(kBlock), 0, st, d_bytes, d_off, d_epos, d_emsg, E, d_ms);
        hipLaunchKernelGGL(k_walk, dim3(gm), dim3(kBlock), 0, st, d_bytes, d_off, n, d_ms, d_tbase, d_tile0, d_epos, d_flat, d_cnt, d_first, d_stat);
    }
    hipLaunchKernelGGL(k_serial, dim3(gm), dim3(kBlock), 0, st, d_bytes, d_off, n, d_flat, d_status, d_cnt, d_first, d_bad);
    excl_scan(ctx, s->wscan, d_cnt, d_cbase, 2 * n);
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
        cv3.bind(work(ctx, s->w3, cv3.bytes() + 1024));
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
}

extern "C" {

int jg_tpset_create(jg_ctx* ctx, uint64_t cap_strings, uint64_t cap_bytes, jg_tpset** out) {
    return jg::guard([&] {
        auto lk_ = jg::lock(ctx);
        JG_REQUIRE(ctx && out, JG_EINVAL, "jg_tpset_create: NULL argument");
        *out = tpset_create(ctx, cap_strings, cap_bytes);
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
        tpset_apply_ops(s, n, op, off, bytes, is_null, result);
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
        cv.bind(work(ctx, s->w3, cv.bytes() + 1024));
        const Store S = s->view();
        hipLaunchKernelGGL(k_lookup_flag, dim3(blocks_for(m)), dim3(kBlock), 0, st, S, from, m, keep, len);
        excl_scan(ctx, s->wscan, keep, ok, m);
        excl_scan(ctx, s->wscan, len, ob, m);
        if (!query) hipLaunchKernelGGL(k_lookup_write, dim3(blocks_for(m)), dim3(kBlock), 0, st, S, from, m, keep, ok, ob, d_ord, d_off, d_bytes, d_null);
        JG_HIP(hipGetLastError());
        const auto [k, kb] = read_totals(ctx, ok + m, ob + m);
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
    return jg::guard([&] {
        auto lk_ = jg::lock(s);
        tpset_merge_json(s, n, off, bytes, mode, bad_msg, partial);
    });
}

int jg_tpset_last_stats(jg_tpset* s, jg_tpset_stats* out) {
    return jg::guard([&] {
        auto lk_ = jg::lock(s);
        JG_REQUIRE(s && out, JG_EINVAL, "jg_tpset_last_stats: NULL argument");
        *out = s->stats;
        out->tile_bytes = kTile;
        out->stage_bytes = encode_stage_bytes();
        out->encode_s = s->encode_s;
    });
}

}  // extern "C"
