// orset_walk_small.hip — ORSet.Add / Remove / Clear batches of at most kWalkSmallMaxOps ops: the record walk of
// orset_walk.hip in ONE launch of ONE workgroup (gfx950).
//
// The multi-launch form costs some forty launches and two mid-call waits whatever the batch size; the batches a node
// makes (at most 1000 commands) are below the size where that pays.  Here the same arithmetic (orset_walk.hpp) runs in
// one workgroup of 1024 threads, one op per thread in each order, with block sorts and block scans over LDS and
// __syncthreads() where the other form has launch boundaries:
//   order    : P1 = (set, op index) and P2 = (set, elem, op index) by stable block radix sorts; Clear epochs, set heads,
//              segment and key heads by block scans
//   classify : first occurrence of a tag in its segment by a loop over the segment (bounded by the cap); the bounds of
//              the stored runs; the stored add tags of those keys expanded into a fixed scratch of kWalkSmallMaxStored
//              items — more than that raises a flag and returns before any output is written (the host then runs the
//              multi-launch form); U0 ranked by (seg, ord, tag) with one block radix sort of integer words
//   scans    : issues, fills and u-adds in one packed scan; the marks both ways; the ord bases in P1 order
//   emit     : each record's rank by (key, tag) counted, not sorted: records before its key by a scan, records of its
//              key below its tag by a loop over the segment (and the stored run's live prefix for U0)
// The host uploads the five input arrays as one packed copy, reads the counter words in one wait, and hands the two
// streams to the same union as the other form.
#include <hipcub/hipcub.hpp>

#include <cstdlib>
#include <cstring>

#include "launch.hpp"
#include "orset_walk_small.hpp"
#include "orset_walk_types.hpp"

namespace {

using jgk::Tag;
using jgk::View;
using jgk::ld_tag;
using jgw::Item;
using jgw::kNone;
using ull = unsigned long long;

constexpr int kT = (int)jgs::kThreads;
constexpr int kIPT = (int)jgs::kItemsPerThread;
static_assert(jgs::kMaxOps <= jgs::kThreads, "one op per thread");

// The counter words (uint64 each) the host reads after the launch.
enum : int { cNextA = 1, cNextR, cKeptA, cKeptR, cCleared, cMaxCleared, cSpanA, cSpanR, cCursor, cErr, cEmitA, cBudget, cStored, cCount = 16 };

struct Args {
    View a, r;
    const unsigned char* in;  // the packed upload (jgs::upload_layout)
    uint32_t n;
    int set_bits, elem_bits, ord_bits;  // the widths of the batch's largest set id and element id and of the store's add ords
    // scratch kept on the store
    ull* bnd;         // [4 kMaxOps] rank bounds of the stored runs, at the key's first position
    Item* items;      // [kMaxStored]
    uint32_t* livex;  // [kMaxStored + 1] items without a tombstone before item j
    // outputs
    uint8_t* res;
    ull *alim, *rlim;
    ull* akey;
    uint4* atag;
    uint32_t* aord;
    ull* rkey;
    uint4* rtag;
    uint32_t* rord;
    uint32_t cap_a, cap_r;
    unsigned* drop;
    uint32_t drop_words;
    ull* cn;
};

using Sort32 = hipcub::BlockRadixSort<uint32_t, kT, 1, uint32_t>;
using Sort64 = hipcub::BlockRadixSort<ull, kT, 1, uint32_t>;
using SortIt = hipcub::BlockRadixSort<ull, kT, kIPT>;
using Scan32 = hipcub::BlockScan<uint32_t, kT>;
using Scan64 = hipcub::BlockScan<ull, kT>;

union Temp {
    typename Sort32::TempStorage s32;
    typename Sort64::TempStorage s64;
    typename SortIt::TempStorage sit;
    typename Scan32::TempStorage c32;
    typename Scan64::TempStorage c64;
};

// The rank bounds of key q's runs in both streams, as jgk::lower_key / upper_key give them.  The two lower bounds are
// searched in one loop, so their loads are in flight together (a search is a chain of dependent misses, some 18 for
// 200,000 records); each upper bound gallops from its lower one, the runs being short against the stream.
__device__ __forceinline__ uint64_t upper_from(const View& v, unsigned long long q, uint64_t from) {
    uint64_t lo = from, b = from, step = 1;
    while (b < v.n && jgk::key_at(v, b) <= q) lo = b + 1, b += step, step <<= 1;
    uint64_t hi = b < v.n ? b : v.n;
    while (lo < hi) {
        const uint64_t m = (lo + hi) >> 1;
        if (jgk::key_at(v, m) <= q) lo = m + 1;
        else hi = m;
    }
    return lo;
}
__device__ __forceinline__ void key_bounds(const View& a, const View& r, unsigned long long q, ull* __restrict__ out) {
    uint64_t la = 0, ha = a.n, lr = 0, hr = r.n;
    while (la < ha || lr < hr) {
        const bool sa = la < ha, sr = lr < hr;
        const uint64_t ma = (la + ha) >> 1, mr = (lr + hr) >> 1;
        const unsigned long long ka = sa ? jgk::key_at(a, ma) : 0ull, kr = sr ? jgk::key_at(r, mr) : 0ull;
        if (sa) {
            if (ka < q) la = ma + 1;
            else ha = ma;
        }
        if (sr) {
            if (kr < q) lr = mr + 1;
            else hr = mr;
        }
    }
    out[0] = la, out[1] = upper_from(a, q, la);
    out[2] = lr, out[3] = upper_from(r, q, lr);
}

__global__ __launch_bounds__(kT) void k_walk_small(const Args A) {
    __shared__ Temp tmp;
    __shared__ ull s_cn[cCount];
    // by op index
    __shared__ uint8_t s_op[kT], s_keep[kT], s_issue_w[kT];
    __shared__ uint16_t s_epoch[kT];
    __shared__ uint32_t s_cntr[kT], s_abase[kT], s_rbase[kT];
    // by position of P1
    __shared__ uint32_t s_s1[kT], s_nclr[kT];
    __shared__ uint16_t s_p1[kT], s_cx[kT];
    // by position of P2
    __shared__ ull s_k2[kT], s_lo2[kT], s_hi2[kT], s_sums[kT], s_ioff[kT + 1];
    __shared__ uint32_t s_kf[kT], s_fr[kT], s_u0n[kT], s_u0x[kT], s_marks[kT], s_revs[kT], s_kax[kT], s_tx[kT];
    __shared__ uint16_t s_p2[kT], s_e2[kT], s_seg[kT], s_kseg[kT];
    __shared__ uint8_t s_op2[kT], s_flag[kT];

    const uint32_t t = threadIdx.x, n = A.n;
    const bool act = t < n;
    const jgs::Upload L = jgs::upload_layout(n);
    const ull* g_lo = reinterpret_cast<const ull*>(A.in + L.lo);
    const ull* g_hi = reinterpret_cast<const ull*>(A.in + L.hi);
    const uint32_t* g_set = reinterpret_cast<const uint32_t*>(A.in + L.set);
    const uint32_t* g_elem = reinterpret_cast<const uint32_t*>(A.in + L.elem);
    const uint8_t* g_op = A.in + L.op;

    const uint32_t my_set = act ? g_set[t] : 0xFFFFFFFFu, my_elem = act ? g_elem[t] : 0xFFFFFFFFu;
    s_op[t] = act ? g_op[t] : 0;
    if (t < cCount) s_cn[t] = 0;
    s_nclr[t] = 0, s_kf[t] = 0, s_u0n[t] = 0, s_fr[t] = kNone;

    // ---- order 1: (set, op index).  The sorts are stable and the idle threads' keys are the largest, so positions
    // [0, n) hold the batch's ops in either order ----
    {
        uint32_t k[1] = {act ? my_set : 0xFFFFFFFFu >> (32 - A.set_bits)}, v[1] = {t};
        Sort32(tmp.s32).Sort(k, v, 0, A.set_bits);
        s_s1[t] = k[0], s_p1[t] = (uint16_t)v[0];
    }
    __syncthreads();
    bool clr_head = false;  // this position is the first of a set the batch Clears
    {
        const uint32_t x = t;
        const uint32_t clr = act && s_op[s_p1[x]] == 3 ? 1u : 0u;
        const uint32_t head = (act && x > 0 && s_s1[x] != s_s1[x - 1]) ? x : 0u;
        uint32_t cx, ss;
        Scan32(tmp.c32).ExclusiveSum(clr, cx);
        __syncthreads();
        Scan32(tmp.c32).InclusiveScan(head, ss, hipcub::Max());
        s_cx[x] = (uint16_t)cx;
        __syncthreads();
        const uint32_t ep = cx - s_cx[ss];  // the Clears of the op's set before it
        if (act) {
            s_epoch[s_p1[x]] = (uint16_t)ep;
            if (clr) atomicAdd(&s_nclr[ss], 1u);
        }
        __syncthreads();
        if (act) {
            const uint32_t c = s_nclr[ss];
            s_keep[s_p1[x]] = ep == c ? 1 : 0;  // no Clear of its set follows
            if (ss == x && c > 0) {
                clr_head = true;
                atomicAdd(&s_cn[cCleared], 1ull);
                atomicMax(&s_cn[cMaxCleared], (ull)s_s1[x]);
            }
        }
    }

    // ---- order 2: (set, elem, op index) = (set, elem, epoch, op index) ----
    {
        const int bits = A.set_bits + A.elem_bits;
        ull k[1] = {act ? jgs::op_key(my_set, my_elem, A.elem_bits) : ~0ull >> (64 - bits)};
        uint32_t v[1] = {t};
        Sort64(tmp.s64).Sort(k, v, 0, bits);
        s_k2[t] = jgs::op_key_wide(k[0], A.elem_bits), s_p2[t] = (uint16_t)v[0];
    }
    __syncthreads();
    const uint32_t p = t;
    const uint32_t i = act ? s_p2[p] : 0u;
    const uint8_t o = act ? s_op[i] : 0;
    const uint32_t e = act ? s_epoch[i] : 0u;
    const ull tlo = act ? g_lo[i] : 0ull, thi = act ? g_hi[i] : 0ull;
    s_e2[p] = (uint16_t)e, s_op2[p] = o, s_lo2[p] = tlo, s_hi2[p] = thi;
    __syncthreads();
    uint32_t seg, kseg;
    {
        const bool kh = act && p > 0 && s_k2[p] != s_k2[p - 1];
        const bool sh = kh || (act && p > 0 && e != s_e2[p - 1]);
        Scan32(tmp.c32).InclusiveScan(sh ? p : 0u, seg, hipcub::Max());
        __syncthreads();
        Scan32(tmp.c32).InclusiveScan(kh ? p : 0u, kseg, hipcub::Max());
        s_seg[p] = (uint16_t)seg, s_kseg[p] = (uint16_t)kseg;
    }
    // kf[key's first position]: 1 a Remove names the key, 2 a read does; fr[...]: the first Remove of its epoch-0 segment
    if (o == 2) {
        atomicOr(&s_kf[kseg], 1u);
        if (e == 0) atomicMin(&s_fr[kseg], p);
    } else if (o == 4) {
        atomicOr(&s_kf[kseg], 2u);
    }
    __syncthreads();

    // ---- classify ----
    const bool fst = o == 1 && !jgs::seen_before(s_op2, s_lo2, s_hi2, seg, p, tlo, thi);
    // the stored runs of every key a Remove or a read names and whose first segment is epoch 0
    ull len = 0, T = 0;
    if (act && kseg == p && s_kf[p] && e == 0) {
        key_bounds(A.a, A.r, s_k2[p], A.bnd + 4 * p);
        len = A.bnd[4 * p + 1] - A.bnd[4 * p];
    }
    {
        ull off;
        Scan64(tmp.c64).ExclusiveSum(len, off, T);
        s_ioff[p] = off;
        if (t == 0) s_ioff[kT] = T;
    }
    __syncthreads();  // (and the bounds written above are visible to the workgroup)
    if (T > jgs::kMaxStored) {  // uniform: nothing has been written but scratch
        if (t < cCount) A.cn[t] = t == cBudget ? 1ull : t == cStored ? T : 0ull;
        return;
    }
    // every stored add tag of those keys: whether it lacks a tombstone (then it is in U0, counted in u0n[p])
    ull ikey[kIPT];
    uint32_t live = 0;
#pragma unroll
    for (int k = 0; k < kIPT; ++k) {
        const uint32_t j = t * kIPT + k;
        ikey[k] = jgs::item_key(jgs::kItemNoSeg, 0u, j, A.ord_bits);
        if (j < T) {
            const uint32_t q = (uint32_t)jgw::last_le(s_ioff, n, j);
            const uint64_t x = jgk::slot_of(A.a, A.bnd[4 * q] + (j - s_ioff[q]));
            const Tag g = ld_tag(A.a.tag + x);
            const bool dead = jgw::has_tag(A.r, A.bnd[4 * q + 2], A.bnd[4 * q + 3], g.lo, g.hi);
            const uint32_t ord = A.a.ord[x];
            A.items[j] = Item{dead ? kNone : q, ord, g.lo, g.hi};
            if (!dead) {
                atomicAdd(&s_u0n[q], 1u);
                ikey[k] = jgs::item_key(q, ord, j, A.ord_bits);
                live |= 1u << k;
                if (A.ord_bits < 32 && (ord >> A.ord_bits)) atomicOr(&s_cn[cErr], 8ull);  // a stored ord not below the stream's next
            }
        }
    }
    {
        uint32_t before;
        Scan32(tmp.c32).ExclusiveSum((uint32_t)__builtin_popcount(live), before);
#pragma unroll
        for (int k = 0; k < kIPT; ++k) {
            A.livex[t * kIPT + k] = before;
            before += (live >> k) & 1u;
        }
        if (t == kT - 1) A.livex[jgs::kMaxStored] = before;
    }
    __syncthreads();
    if (T) {  // uniform; U0 in (seg, ord, tag) order: thread t then holds sorted places kIPT t ..
        SortIt(tmp.sit).Sort(ikey, 0, jgs::item_key_bits(A.ord_bits));
        __syncthreads();
    }
    {
        uint32_t u0x;
        Scan32(tmp.c32).ExclusiveSum(s_u0n[p], u0x);
        s_u0x[p] = u0x;
    }
    const uint32_t f = s_kf[kseg];
    const bool store = e == 0 && f != 0;
    const jgw::Base base = jgw::base_of(kseg, act && store, A.bnd, s_u0n[kseg]);
    bool is = false, fl = false;
    {
        bool w = false;
        if (o == 1) {
            bool in_a = false, in_r = false;
            if (fst && store) {
                in_a = jgw::has_tag(A.a, A.bnd[4 * kseg], A.bnd[4 * kseg + 1], tlo, thi);
                in_r = jgw::has_tag(A.r, A.bnd[4 * kseg + 2], A.bnd[4 * kseg + 3], tlo, thi);
            }
            is = fst && !in_a;
            fl = is && in_r;
            w = (f & 1u) ? is : fst;  // the stored runs enter the write state only under a Remove of the key
        }
        if (act) s_issue_w[i] = w ? 1 : 0;
    }
    const bool ua = is && !fl;

    // ---- scans ----
    __syncthreads();
    {
        ull sums;
        Scan64(tmp.c64).ExclusiveSum(jgs::pack3(is, fl, ua), sums);
        s_sums[p] = sums;
        __syncthreads();
        uint32_t m;
        Scan32(tmp.c32).InclusiveScan(act ? jgw::mark(p, seg == p, o == 2) : 0u, m, hipcub::Max());
        s_marks[p] = m;
        s_tx[p] = 0;  // (borrowed for the reversed marks' inputs)
        __syncthreads();
        if (act) s_tx[jgw::rev_slot(n, p)] = jgw::rev_mark(n, p, o == 2);
        __syncthreads();
        Scan32(tmp.c32).InclusiveScan(s_tx[t], m, hipcub::Max());
        s_revs[t] = m;
    }
    __syncthreads();
    // results, and each Remove's tombstone count
    const uint32_t q_rm = act ? jgw::prev_remove(s_marks, p, seg) : kNone;
    const ull sum_p = s_sums[p], sum_s = s_sums[seg], sum_q = q_rm != kNone ? s_sums[q_rm] : sum_s;
    const uint32_t ua_p = jgs::sum_ua(sum_p) - jgs::sum_ua(sum_s), ua_q = jgs::sum_ua(sum_q) - jgs::sum_ua(sum_s);
    if (act) {
        uint8_t out = 1;
        uint32_t c = 0;
        if (o == 2 || o == 4) {
            const jgw::State st = jgw::state_at(base, jgs::sum_is(sum_p) - jgs::sum_is(sum_s), jgs::sum_fl(sum_p) - jgs::sum_fl(sum_s), ua_p,
                                                q_rm != kNone, ua_q);
            out = jgw::present(g_elem[i], st) ? 1 : 0;
            if (o == 2) {
                c = (uint32_t)st.u;
                if (c && s_keep[i]) atomicAdd(&s_cn[cKeptR], (ull)c);
            }
        }
        A.res[i] = out;
        s_cntr[i] = c;
    }
    __syncthreads();
    // order 1: the limits right after each op (batch ords, not rebased), each op's first ord, the totals and the spans
    {
        const uint32_t x = t, i1 = act ? s_p1[x] : 0u;
        const ull va = act ? s_issue_w[i1] : 0u, vr = act ? s_cntr[i1] : 0u;
        ull sx;
        Scan64(tmp.c64).ExclusiveSum(va | (vr << 32), sx);
        if (act) {
            const ull a0 = sx & 0xFFFFFFFFull, r0 = sx >> 32, a1 = a0 + va, r1 = r0 + vr;
            A.alim[i1] = a1, A.rlim[i1] = r1;
            s_abase[i1] = (uint32_t)a0, s_rbase[i1] = (uint32_t)r0;
            if (s_keep[i1]) {
                if (a1 > a0) atomicMax(&s_cn[cSpanA], a1);
                if (r1 > r0) atomicMax(&s_cn[cSpanR], r1);
            }
            if (x + 1 == n) s_cn[cNextA] = a1, s_cn[cNextR] = r1;
        }
    }
    __syncthreads();

    // ---- emit: the kept add records in (key, tag) order ----
    {
        const bool ka = act && o == 1 && s_issue_w[i] && s_keep[i];
        uint32_t kax, n_add;
        Scan32(tmp.c32).ExclusiveSum(ka ? 1u : 0u, kax, n_add);
        s_kax[p] = kax, s_flag[p] = ka ? 1 : 0;
        __syncthreads();
        if (ka) {  // the kept Adds of a key are those of its last segment, each tag once
            const uint32_t at = s_kax[seg] + jgs::rank_in_segment(s_flag, s_seg, s_lo2, s_hi2, n, seg, tlo, thi);
            if (at < A.cap_a) {
                A.akey[at] = s_k2[p];
                A.atag[at] = jgk::to_u4(Tag{tlo, thi});
                A.aord[at] = s_abase[i];
                atomicAdd(&s_cn[cEmitA], 1ull);
            } else {
                atomicOr(&s_cn[cErr], 1ull);
            }
        }
        if (t == 0) s_cn[cKeptA] = n_add;
        __syncthreads();
    }
    // ---- emit: the tombstones in (key, tag) order.  A u-add is tombstoned by the next Remove of its segment; the stored
    // tags of U0, in (ord, tag) order, by the first Remove of the key's epoch-0 segment ----
    {
        bool em = false;
        uint32_t ir = 0;
        if (ua) {
            const uint32_t r = jgw::next_remove(s_revs, n, p);
            if (r != kNone && s_seg[r] == seg) {
                ir = s_p2[r];
                em = s_keep[ir] != 0;
            }
        }
        uint32_t cnt = em ? 1u : 0u;
        if (act && kseg == p) {
            const uint32_t r = s_fr[p];
            if (r != kNone && s_keep[s_p2[r]]) cnt += s_u0n[p];
        }
        uint32_t tx;
        Scan32(tmp.c32).ExclusiveSum(cnt, tx);
        s_tx[p] = tx, s_flag[p] = em ? 1 : 0;
        __syncthreads();
        if (em) {
            uint32_t rank = jgs::rank_in_segment(s_flag, s_seg, s_lo2, s_hi2, n, seg, tlo, thi);
            if (store && s_u0n[kseg]) {  // the key's U0 tags below this one: the live prefix of its stored run
                const uint64_t a0 = A.bnd[4 * kseg], lb = jgw::lower_tag(A.a, a0, A.bnd[4 * kseg + 1], tlo, thi);
                const uint32_t j0 = (uint32_t)s_ioff[kseg];
                rank += A.livex[j0 + (uint32_t)(lb - a0)] - A.livex[j0];
            }
            const uint32_t at = s_tx[kseg] + rank;
            if (at < A.cap_r) {
                A.rkey[at] = s_k2[p];
                A.rtag[at] = jgk::to_u4(Tag{tlo, thi});
                A.rord[at] = s_rbase[ir] + (uint32_t)jgw::uadd_slot(base, ua_p, q_rm != kNone, ua_q);
                atomicAdd(&s_cn[cCursor], 1ull);
            } else {
                atomicOr(&s_cn[cErr], 2ull);
            }
        }
#pragma unroll
        for (int k = 0; k < kIPT; ++k) {
            const uint32_t sg = jgs::item_seg(ikey[k], A.ord_bits);
            if (sg == jgs::kItemNoSeg) continue;
            const uint32_t r = s_fr[sg];
            if (r == kNone) continue;
            const uint32_t ir0 = s_p2[r];
            if (!s_keep[ir0]) continue;
            const uint32_t j = jgs::item_idx(ikey[k]), x = t * kIPT + k;
            const Item it = A.items[j];
            const uint32_t rank = A.livex[j] - A.livex[(uint32_t)s_ioff[sg]] + jgs::rank_in_segment(s_flag, s_seg, s_lo2, s_hi2, n, sg, it.lo, it.hi);
            const uint32_t at = s_tx[sg] + rank;
            if (at < A.cap_r) {
                A.rkey[at] = s_k2[sg];
                A.rtag[at] = jgk::to_u4(Tag{it.lo, it.hi});
                A.rord[at] = s_rbase[ir0] + (x - s_u0x[sg]);
                atomicAdd(&s_cn[cCursor], 1ull);
            } else {
                atomicOr(&s_cn[cErr], 2ull);
            }
        }
    }
    // the union's drop bitmap: one bit per Cleared set
    if (clr_head) {
        const uint32_t s = s_s1[t];
        if ((s >> 5) < A.drop_words) atomicOr(A.drop + (s >> 5), 1u << (s & 31));
        else atomicOr(&s_cn[cErr], 4ull);
    }
    __syncthreads();
    if (t < cCount) A.cn[t] = t == cStored ? T : s_cn[t];
}

}  // namespace

namespace jg {

int orset_walk_small_default() {
    static const int mode = [] {
        const char* e = std::getenv("JANUS_ORSET_WALK_SMALL");
        if (e && !std::strcmp(e, "off")) return 0;
        if (e && !std::strcmp(e, "on")) return 1;
        return 2;
    }();
    return mode;
}

void orset_walk_small_free(jg_orset* batch) { delete batch; }

bool orset_walk_small(jg_orset* s, uint64_t n, const uint32_t* set, const uint32_t* elem, const uint8_t* op, const uint64_t* tag_lo,
                      const uint64_t* tag_hi, uint8_t* result, uint64_t* add_lim, uint64_t* rem_lim) {
    static const bool tr = std::getenv("JANUS_TRACE_APPLY") != nullptr;
    jg_ctx* ctx = s->ctx;
    hipStream_t st = ctx->stream;
    JG_REQUIRE(n >= 1 && n <= jgs::kMaxOps, JG_EINVAL, "jg_orset_apply_ops: %llu ops do not fit the one-launch walk", (unsigned long long)n);

    // phases on events, under the flag only
    constexpr int kEv = 5;
    hipEvent_t ev[kEv] = {};
    int n_ev = 0;
    auto mark = [&] {
        if (!tr) return;
        JG_HIP(hipEventCreate(&ev[n_ev]));
        JG_HIP(hipEventRecord(ev[n_ev], st));
        ++n_ev;
    };
    struct EvGuard {
        hipEvent_t* e;
        ~EvGuard() {
            for (int i = 0; i < kEv; ++i)
                if (e[i]) (void)hipEventDestroy(e[i]);
        }
    } ev_guard{ev};

    // ---- the store's fixed scratch and batch buffers, allocated once ----
    constexpr uint64_t kCapA = jgs::kMaxOps, kCapR = (uint64_t)jgs::kMaxOps + jgs::kMaxStored;
    Args A{};
    unsigned char* d_in;
    ull* cn;
    Layout W;
    W.add(cn, cCount), W.add(A.bnd, 4 * jgs::kMaxOps), W.add(A.alim, jgs::kMaxOps), W.add(A.rlim, jgs::kMaxOps), W.add(A.items, jgs::kMaxStored);
    W.add(A.livex, jgs::kMaxStored + 1), W.add(d_in, jgs::upload_layout(jgs::kMaxOps).bytes), W.add(A.res, jgs::kMaxOps);
    ensure(s->walk_small_ws, W.bytes());
    W.bind(s->walk_small_ws.p);
    if (!s->walk_small_batch) {
        s->walk_small_batch = new jg_orset;
        s->walk_small_batch->ctx = ctx;
        s->walk_small_batch->add.reserve_records(kCapA);
        s->walk_small_batch->rem.reserve_records(kCapR);
    }
    jg_orset* batch = s->walk_small_batch;

    // ---- upload: the five arrays as one packed copy from the context's page-locked write area ----
    const jgs::Upload L = jgs::upload_layout(n);
    static_assert(jgs::upload_layout(jgs::kMaxOps).bytes <= kPinBytes - kPinRead, "a packed batch fits the page-locked write area");
    char* pin = static_cast<char*>(ctx->hstat) + kPinRead;
    std::memcpy(pin + L.lo, tag_lo, n * 8);
    std::memcpy(pin + L.hi, tag_hi, n * 8);
    std::memcpy(pin + L.set, set, n * 4);
    std::memcpy(pin + L.elem, elem, n * 4);
    std::memcpy(pin + L.op, op, n);
    // the Clear drop bitmap's size is known from the ops themselves
    // and the widths the sorts run over
    bool any_clear = false;
    uint32_t max_cleared = 0, max_set = 0, max_elem = 0;
    for (uint64_t i = 0; i < n; ++i) {
        max_set = std::max(max_set, set[i]), max_elem = std::max(max_elem, elem[i]);
        if (op[i] == 3) any_clear = true, max_cleared = std::max(max_cleared, set[i]);
    }
    const uint32_t words = any_clear ? (max_cleared >> 5) + 1 : 0;
    DevBuf big_drop;  // a bitmap past 1 MiB is not kept on the store
    unsigned* d_drop = nullptr;
    mark();
    if (words) {
        const size_t bytes = (size_t)words * 4;
        if (bytes <= (1u << 20)) {
            ensure(s->walk_small_drop, bytes);
            d_drop = s->walk_small_drop.as<unsigned>();
        } else {
            big_drop.alloc(bytes);
            d_drop = big_drop.as<unsigned>();
        }
        JG_HIP(hipMemsetAsync(d_drop, 0, bytes, st));
    }
    JG_HIP(hipMemcpyAsync(d_in, pin, L.bytes, hipMemcpyHostToDevice, st));
    mark();  // upload

    // ---- the walk ----
    A.a = orset_view(s->add), A.r = orset_view(s->rem);
    A.in = d_in, A.n = (uint32_t)n;
    A.set_bits = jgs::bits_for(max_set), A.elem_bits = jgs::bits_for(max_elem);
    A.ord_bits = std::min(32, jgs::bits_for(s->add.next ? s->add.next - 1 : 0));  // every stored ord is below next
    A.akey = batch->add.key.as<ull>(), A.atag = batch->add.tag.as<uint4>(), A.aord = batch->add.ord.as<uint32_t>();
    A.rkey = batch->rem.key.as<ull>(), A.rtag = batch->rem.tag.as<uint4>(), A.rord = batch->rem.ord.as<uint32_t>();
    A.cap_a = (uint32_t)kCapA, A.cap_r = (uint32_t)kCapR;
    A.drop = d_drop, A.drop_words = words;
    A.cn = cn;
    hipLaunchKernelGGL(k_walk_small, dim3(1), dim3(kT), 0, st, A);
    JG_HIP(hipGetLastError());
    pin_get(ctx, 0, cn, cCount * 8);
    pin_sync(ctx);
    mark();  // kernel
    unsigned long long h[cCount];
    std::memcpy(h, pin_at(ctx, 0), sizeof h);
    if (h[cBudget]) {  // more stored tags than the scratch holds: nothing was written, the multi-launch form takes the batch
        s->walk_small_stats[2] += 1;
        return false;
    }
    const uint64_t n_add = h[cKeptA], n_rem = h[cKeptR];
    s->walk_stats[0] += 1;
    s->walk_stats[2] += n;
    s->walk_small_stats[0] += 1;
    s->walk_small_stats[1] += n;
    auto copy_out = [&](uint64_t base_a, uint64_t base_r) {
        JG_HIP(hipMemcpyAsync(result, A.res, n, hipMemcpyDeviceToHost, st));
        if (add_lim) {
            JG_HIP(hipMemcpyAsync(add_lim, A.alim, n * 8, hipMemcpyDeviceToHost, st));
            JG_HIP(hipMemcpyAsync(rem_lim, A.rlim, n * 8, hipMemcpyDeviceToHost, st));
        }
        JG_HIP(hipStreamSynchronize(st));
        if (add_lim)
            for (uint64_t i = 0; i < n; ++i) add_lim[i] += base_a, rem_lim[i] += base_r;
    };
    JG_REQUIRE(h[cErr] == 0 && h[cCursor] == n_rem && h[cEmitA] == n_add && (h[cCleared] != 0) == any_clear &&
                   (!any_clear || h[cMaxCleared] == max_cleared),
               JG_ESTATE, "jg_orset_apply_ops: the one-launch walk emitted %llu + %llu records for %llu + %llu counted (flag %llu)", h[cEmitA],
               h[cCursor], (unsigned long long)n_add, (unsigned long long)n_rem, h[cErr]);
    if (n_add == 0 && n_rem == 0 && h[cCleared] == 0) {
        copy_out(s->add.next, s->rem.next);
        return true;
    }
    JG_REQUIRE(h[cNextA] < 0xFFFFFFFFull && h[cNextR] < 0xFFFFFFFFull, JG_EINVAL, "jg_orset_apply_ops: too many records in one batch");

    // ---- union ----
    set_dense(ctx, batch->add, n_add);
    set_dense(ctx, batch->rem, n_rem);
    batch->add.next = h[cSpanA];
    batch->rem.next = h[cSpanR];
    uint64_t base_a = 0, base_r = 0;
    orset_walk_union(s, batch, jgk::Drop{d_drop, words}, &base_a, &base_r);
    mark();  // union
    copy_out(base_a, base_r);
    mark();  // copies out
    if (tr && n_ev == kEv) {
        float ms[kEv - 1];
        JG_HIP(hipEventSynchronize(ev[kEv - 1]));
        for (int i = 0; i + 1 < kEv; ++i) JG_HIP(hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
        std::fprintf(stderr, "orset apply_ops in one launch (%llu ops, %llu+%llu records, %llu stored tags read): upload %.3f ms, kernel %.3f ms, "
                     "union %.3f ms, copies out %.3f ms\n", (unsigned long long)n, (unsigned long long)n_add, (unsigned long long)n_rem, h[cStored],
                     ms[0], ms[1], ms[2], ms[3]);
    }
    return true;
}

}  // namespace jg

extern "C" {

int jg_orset_set_walk_small(jg_orset* s, int mode) {
    return jg::guard([&] {
        auto lk_ = jg::lock(s);
        JG_REQUIRE(s, JG_EINVAL, "jg_orset_set_walk_small: store is NULL");
        JG_REQUIRE(mode >= 0 && mode <= 2, JG_EINVAL, "jg_orset_set_walk_small: mode %d is not 0 (off), 1 (on) or 2 (auto)", mode);
        s->walk_small_mode = mode;
    });
}

int jg_orset_walk_small_stats(jg_orset* s, uint64_t out[6]) {
    return jg::guard([&] {
        auto lk_ = jg::lock(s);
        JG_REQUIRE(s && out, JG_EINVAL, "jg_orset_walk_small_stats: NULL argument");
        out[0] = s->walk_small_stats[0], out[1] = s->walk_small_stats[1], out[2] = s->walk_small_stats[2], out[3] = 0;
        out[4] = jg::kWalkSmallMaxOps, out[5] = jg::kWalkSmallMaxStored;
    });
}

}  // extern "C"
