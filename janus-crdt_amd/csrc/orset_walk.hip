// orset_walk.hip — ORSet.Add / Remove / Clear batches: the record walk on the device (gfx950).
//
// orset.hip's apply_ops() replays a batch over std::set states on the host after fetching the stored runs.  This
// unit computes the same results, records, ords and limits with sorts and prefix sums (orset_walk.hpp states the
// form), and hands the two record streams to the same union.  Nothing of the store crosses to the host.
//   order    : P1 = ops by (set, op index), P2 = ops by (set, elem, op index) (stable radix sorts); the Clear epoch
//              of an op = Clears of its set before it, so P2 is also (set, elem, epoch, op index) order
//   classify : first occurrence of a tag within (key, epoch) (a merge sort of the Adds by (key, epoch, tag, index));
//              the bounds of the stored runs of every key a Remove or a read names; each epoch-0 Add's tag searched
//              in them; the stored add tags that lack a tombstone (U0), ranked by (ord, tag)
//   scans    : issues, fills, u-adds; the last Remove before and the next Remove after a position
//   emit     : results; add records in (key, tag) order straight from the tag sort; tombstones appended and sorted
//   union    : orset.hip's ensure_ord_room + merge_into over device streams
#include <hipcub/hipcub.hpp>

#include <cstdlib>
#include <cstring>

#include "launch.hpp"
#include "orset_walk_types.hpp"

namespace {

constexpr int kWB = 256;

using jgk::Tag;
using jgk::View;
using jgk::ld_tag;

#define JGW_EACH(i, n) for (uint64_t i = (uint64_t)blockIdx.x * kWB + threadIdx.x; i < (n); i += (uint64_t)gridDim.x * kWB)

using jgw::Item;
using jgw::ItemLess;
using jgw::TagLess;
using jgw::TagRec;
using jgw::Tomb;
using jgw::TombLess;
using jgw::has_tag;

// The counters (uint64 each, zeroed per call).
enum : int { cNextA = 1, cNextR, cKeptA, cKeptR, cCleared, cMaxCleared, cSpanA, cSpanR, cCursor, cErr, cCount = 16 };

__global__ __launch_bounds__(kWB) void k_prep(const uint32_t* __restrict__ set, const uint32_t* __restrict__ elem, uint64_t n,
                                              unsigned long long* __restrict__ key, uint32_t* __restrict__ idx) {
    JGW_EACH(i, n) {
        key[i] = ((unsigned long long)set[i] << 32) | elem[i];
        idx[i] = (uint32_t)i;
    }
}

// P1 order: Clear flags and set heads.
__global__ __launch_bounds__(kWB) void k_ord1_flags(const uint32_t* __restrict__ s1, const uint32_t* __restrict__ p1, const uint8_t* __restrict__ op,
                                                    uint64_t n, uint32_t* __restrict__ clr, uint32_t* __restrict__ head) {
    JGW_EACH(x, n) {
        clr[x] = op[p1[x]] == 3 ? 1u : 0u;
        head[x] = (x > 0 && s1[x] != s1[x - 1]) ? (uint32_t)x : 0u;
    }
}
// epoch[i] = Clears of i's set before it; nclr[set's first position] = the set's Clears.
__global__ __launch_bounds__(kWB) void k_epoch(const uint32_t* __restrict__ p1, const uint32_t* __restrict__ clr, const uint32_t* __restrict__ cx,
                                               const uint32_t* __restrict__ ss, uint64_t n, uint32_t* __restrict__ epoch, uint32_t* __restrict__ nclr) {
    JGW_EACH(x, n) {
        const uint32_t h = ss[x];
        epoch[p1[x]] = cx[x] - cx[h];
        if (clr[x]) atomicAdd(nclr + h, 1u);
    }
}
// keep[i]: i's records survive (no Clear of its set follows); the cleared sets counted; the tag sort's input.
__global__ __launch_bounds__(kWB) void k_keep(const uint32_t* __restrict__ s1, const uint32_t* __restrict__ p1, const uint32_t* __restrict__ ss,
                                              const uint32_t* __restrict__ nclr, const uint32_t* __restrict__ epoch, const uint8_t* __restrict__ op,
                                              const unsigned long long* __restrict__ key, const unsigned long long* __restrict__ lo,
                                              const unsigned long long* __restrict__ hi, uint64_t n, uint8_t* __restrict__ keep,
                                              TagRec* __restrict__ ts, unsigned long long* __restrict__ cn) {
    JGW_EACH(x, n) {
        const uint32_t i = p1[x], h = ss[x], c = nclr[h];
        keep[i] = epoch[i] == c ? 1 : 0;
        if (h == x && c > 0) {
            atomicAdd(cn + cCleared, 1ull);
            atomicMax(cn + cMaxCleared, (unsigned long long)s1[x]);
        }
        const uint32_t cls = op[i] == 1 ? 0u : 1u;
        ts[i] = TagRec{key[i], cls ? 0ull : lo[i], cls ? 0ull : hi[i], (cls << 31) | epoch[i], i};
    }
}
// P2 order: the epochs gathered, heads of segments (key, epoch) and of keys.
__global__ __launch_bounds__(kWB) void k_ord2_flags(const unsigned long long* __restrict__ k2, const uint32_t* __restrict__ p2,
                                                    const uint32_t* __restrict__ epoch, uint64_t n, uint32_t* __restrict__ e2, uint32_t* __restrict__ hseg,
                                                    uint32_t* __restrict__ hkey) {
    JGW_EACH(p, n) {
        const uint32_t e = epoch[p2[p]];
        e2[p] = e;
        const bool kh = p > 0 && k2[p] != k2[p - 1];
        const bool sh = kh || (p > 0 && e != epoch[p2[p - 1]]);
        hkey[p] = kh ? (uint32_t)p : 0u;
        hseg[p] = sh ? (uint32_t)p : 0u;
    }
}
// kf[key's first position]: 1 a Remove names the key, 2 a read does; fr[...]: the first Remove of its epoch-0 segment.
__global__ __launch_bounds__(kWB) void k_key_flags(const uint32_t* __restrict__ p2, const uint8_t* __restrict__ op, const uint32_t* __restrict__ e2,
                                                   const uint32_t* __restrict__ kseg, uint64_t n, uint32_t* __restrict__ kf, uint32_t* __restrict__ fr) {
    JGW_EACH(p, n) {
        const uint8_t o = op[p2[p]];
        if (o == 2) {
            atomicOr(kf + kseg[p], 1u);
            if (e2[p] == 0) atomicMin(fr + kseg[p], (uint32_t)p);
        } else if (o == 4) {
            atomicOr(kf + kseg[p], 2u);
        }
    }
}
// first[i]: Add i is the first of its tag in its (key, epoch).
__global__ __launch_bounds__(kWB) void k_first(const TagRec* __restrict__ ts, uint64_t n, uint8_t* __restrict__ first) {
    JGW_EACH(x, n) {
        const TagRec t = ts[x];
        bool f = true;
        if (x > 0) {
            const TagRec q = ts[x - 1];
            f = !(q.key == t.key && q.epoch_cls == t.epoch_cls && q.lo == t.lo && q.hi == t.hi);
        }
        first[t.idx] = f ? 1 : 0;
    }
}
// The stored runs of every key a Remove or a read names and whose first segment is epoch 0: bnd[4p..] at the key's
// first position p, len[p] = its stored add tags (0 elsewhere; len[n] = 0).
__global__ __launch_bounds__(kWB) void k_bounds(View a, View r, const unsigned long long* __restrict__ k2, const uint32_t* __restrict__ kseg,
                                                const uint32_t* __restrict__ e2, const uint32_t* __restrict__ kf, uint64_t n,
                                                unsigned long long* __restrict__ bnd, unsigned long long* __restrict__ len) {
    JGW_EACH(p, n + 1) {
        unsigned long long l = 0;
        if (p < n && kseg[p] == p && kf[p] && e2[p] == 0) {
            const unsigned long long key = k2[p];
            const uint64_t a0 = jgk::lower_key(a, key), a1 = jgk::upper_key(a, key);
            bnd[4 * p + 0] = a0, bnd[4 * p + 1] = a1;
            bnd[4 * p + 2] = jgk::lower_key(r, key), bnd[4 * p + 3] = jgk::upper_key(r, key);
            l = a1 - a0;
        }
        len[p] = l;
    }
}
// Every stored add tag of those keys: whether it lacks a tombstone (then it is in U0, counted in u0n[p]).
__global__ __launch_bounds__(kWB) void k_items(View a, View r, const unsigned long long* __restrict__ ioff, const unsigned long long* __restrict__ bnd,
                                               uint64_t n, uint64_t T, Item* __restrict__ it, uint32_t* __restrict__ u0n) {
    JGW_EACH(j, T) {
        const uint64_t p = jgw::last_le(ioff, n, j);
        const uint64_t x = jgk::slot_of(a, bnd[4 * p] + (j - ioff[p]));
        const Tag g = ld_tag(a.tag + x);
        const bool dead = has_tag(r, bnd[4 * p + 2], bnd[4 * p + 3], g.lo, g.hi);
        it[j] = Item{dead ? jgw::kNone : (uint32_t)p, a.ord[x], g.lo, g.hi};
        if (!dead) atomicAdd(u0n + p, 1u);
    }
}

__device__ __forceinline__ jgw::Base base_of(uint32_t ks, bool store, const unsigned long long* __restrict__ bnd, const uint32_t* __restrict__ u0n) {
    return jgw::base_of(ks, store, bnd, store ? u0n[ks] : 0u);
}

// Per position of P2: the Add's flags (1 issues, 2 fills, 4 u-add as the state the Removes and reads see has it; issue_w:
// it issues a record), the scans' inputs.
__global__ __launch_bounds__(kWB) void k_classify(View a, View r, const uint32_t* __restrict__ p2, const uint8_t* __restrict__ op,
                                                  const unsigned long long* __restrict__ lo, const unsigned long long* __restrict__ hi,
                                                  const uint32_t* __restrict__ e2, const uint32_t* __restrict__ seg, const uint32_t* __restrict__ kseg,
                                                  const uint32_t* __restrict__ kf, const uint8_t* __restrict__ first,
                                                  const unsigned long long* __restrict__ bnd, uint64_t n, uint8_t* __restrict__ cls,
                                                  uint8_t* __restrict__ issue_w, uint32_t* __restrict__ v_is, uint32_t* __restrict__ v_fl,
                                                  uint32_t* __restrict__ v_ua, uint32_t* __restrict__ v_mark, uint32_t* __restrict__ v_rev) {
    JGW_EACH(p, n) {
        const uint32_t i = p2[p], ks = kseg[p], f = kf[ks];
        const uint8_t o = op[i];
        bool is = false, fl = false, w = false;
        if (o == 1) {
            const bool fst = first[i] != 0, store = e2[p] == 0 && f != 0;
            bool in_a = false, in_r = false;
            if (fst && store) {
                in_a = has_tag(a, bnd[4 * (uint64_t)ks], bnd[4 * (uint64_t)ks + 1], lo[i], hi[i]);
                in_r = has_tag(r, bnd[4 * (uint64_t)ks + 2], bnd[4 * (uint64_t)ks + 3], lo[i], hi[i]);
            }
            is = fst && !in_a;
            fl = is && in_r;
            w = (f & 1u) ? is : fst;  // the stored runs enter the write state only under a Remove of the key
        }
        cls[p] = (is ? 1 : 0) | (fl ? 2 : 0) | (is && !fl ? 4 : 0);
        issue_w[i] = w ? 1 : 0;
        v_is[p] = is, v_fl[p] = fl, v_ua[p] = is && !fl;
        v_mark[p] = jgw::mark((uint32_t)p, seg[p] == p, o == 2);
        v_rev[jgw::rev_slot((uint32_t)n, (uint32_t)p)] = jgw::rev_mark((uint32_t)n, (uint32_t)p, o == 2);
    }
}

struct Scans {
    const uint32_t *isx, *flx, *uax, *marks, *revs;  // exclusive sums of the three flags; scanned marks both ways
};

// Results, and each Remove's tombstone count.
__global__ __launch_bounds__(kWB) void k_eval(const uint32_t* __restrict__ p2, const uint8_t* __restrict__ op, const uint32_t* __restrict__ elem,
                                              const uint32_t* __restrict__ e2, const uint32_t* __restrict__ seg, const uint32_t* __restrict__ kseg,
                                              const uint32_t* __restrict__ kf, const unsigned long long* __restrict__ bnd, const uint32_t* __restrict__ u0n,
                                              Scans sc, const uint8_t* __restrict__ keep, uint64_t n, uint8_t* __restrict__ res,
                                              unsigned long long* __restrict__ cnt_r, unsigned long long* __restrict__ cn) {
    JGW_EACH(p, n) {
        const uint32_t i = p2[p];
        const uint8_t o = op[i];
        uint8_t out = 1;
        unsigned long long c = 0;
        if (o == 2 || o == 4) {
            const uint32_t s = seg[p], ks = kseg[p];
            const jgw::Base b = base_of(ks, e2[p] == 0 && kf[ks] != 0, bnd, u0n);
            const uint32_t q = jgw::prev_remove(sc.marks, (uint32_t)p, s);
            const jgw::State st = jgw::state_at(b, sc.isx[p] - sc.isx[s], sc.flx[p] - sc.flx[s], sc.uax[p] - sc.uax[s], q != jgw::kNone,
                                                q != jgw::kNone ? sc.uax[q] - sc.uax[s] : 0);
            out = jgw::present(elem[i], st) ? 1 : 0;
            if (o == 2) {
                c = st.u;
                if (c && keep[i]) atomicAdd(cn + cKeptR, c);
            }
        }
        res[i] = out;
        cnt_r[i] = c;
    }
}
// P1 order: the records each op issues.
__global__ __launch_bounds__(kWB) void k_ord1_counts(const uint32_t* __restrict__ p1, const uint8_t* __restrict__ issue_w,
                                                     const unsigned long long* __restrict__ cnt_r, uint64_t n, unsigned long long* __restrict__ va,
                                                     unsigned long long* __restrict__ vr) {
    JGW_EACH(x, n) {
        const uint32_t i = p1[x];
        va[x] = issue_w[i];
        vr[x] = cnt_r[i];
    }
}
// The limits right after each op (batch ords, not yet rebased), each op's first ord, the totals and the kept records' spans.
__global__ __launch_bounds__(kWB) void k_lims(const uint32_t* __restrict__ p1, const unsigned long long* __restrict__ va,
                                              const unsigned long long* __restrict__ vr, const unsigned long long* __restrict__ ax,
                                              const unsigned long long* __restrict__ rx, const uint8_t* __restrict__ keep, uint64_t n,
                                              unsigned long long* __restrict__ alim, unsigned long long* __restrict__ rlim,
                                              unsigned long long* __restrict__ abase, unsigned long long* __restrict__ rbase,
                                              unsigned long long* __restrict__ cn) {
    JGW_EACH(x, n) {
        const uint32_t i = p1[x];
        const unsigned long long a0 = ax[x], r0 = rx[x], a1 = a0 + va[x], r1 = r0 + vr[x];
        alim[i] = a1, rlim[i] = r1;
        abase[i] = a0, rbase[i] = r0;
        if (keep[i]) {
            if (a1 > a0) atomicMax(cn + cSpanA, a1);
            if (r1 > r0) atomicMax(cn + cSpanR, r1);
        }
        if (x + 1 == n) cn[cNextA] = a1, cn[cNextR] = r1;
    }
}
// Tag-sort order: the Adds whose record is kept.
__global__ __launch_bounds__(kWB) void k_add_flags(const TagRec* __restrict__ ts, const uint8_t* __restrict__ issue_w, const uint8_t* __restrict__ keep,
                                                   uint64_t n, uint32_t* __restrict__ ka) {
    JGW_EACH(x, n) {
        const TagRec t = ts[x];
        ka[x] = (t.epoch_cls >> 31) == 0 && issue_w[t.idx] && keep[t.idx];
    }
}
__global__ __launch_bounds__(kWB) void k_emit_add(const TagRec* __restrict__ ts, const uint32_t* __restrict__ ka, const uint32_t* __restrict__ kax,
                                                  const unsigned long long* __restrict__ abase, uint64_t n, uint64_t cap,
                                                  unsigned long long* __restrict__ key, uint4* __restrict__ tag, uint32_t* __restrict__ ord,
                                                  unsigned long long* __restrict__ cn) {
    JGW_EACH(x, n) {
        if (!ka[x]) continue;
        const TagRec t = ts[x];
        const uint64_t o = kax[x];
        if (o >= cap) { atomicOr(cn + cErr, 1ull); continue; }
        key[o] = t.key;
        tag[o] = jgk::to_u4(Tag{t.lo, t.hi});
        ord[o] = (uint32_t)abase[t.idx];
    }
}
// A u-add is tombstoned by the next Remove of its segment.
__global__ __launch_bounds__(kWB) void k_emit_uadd(const unsigned long long* __restrict__ k2, const uint32_t* __restrict__ p2,
                                                   const unsigned long long* __restrict__ lo, const unsigned long long* __restrict__ hi,
                                                   const uint8_t* __restrict__ cls, const uint32_t* __restrict__ e2, const uint32_t* __restrict__ seg,
                                                   const uint32_t* __restrict__ kseg, const uint32_t* __restrict__ kf,
                                                   const unsigned long long* __restrict__ bnd, const uint32_t* __restrict__ u0n, Scans sc,
                                                   const uint8_t* __restrict__ keep, const unsigned long long* __restrict__ rbase, uint64_t n, uint64_t cap,
                                                   Tomb* __restrict__ out, unsigned long long* __restrict__ cn) {
    JGW_EACH(p, n) {
        if (!(cls[p] & 4)) continue;
        const uint32_t s = seg[p];
        const uint32_t r = jgw::next_remove(sc.revs, (uint32_t)n, (uint32_t)p);
        if (r == jgw::kNone || seg[r] != s) continue;
        const uint32_t ir = p2[r];
        if (!keep[ir]) continue;
        const uint32_t ks = kseg[p], i = p2[p];
        const jgw::Base b = base_of(ks, e2[p] == 0 && kf[ks] != 0, bnd, u0n);
        const uint32_t q = jgw::prev_remove(sc.marks, (uint32_t)p, s);
        const uint64_t at = jgw::uadd_slot(b, sc.uax[p] - sc.uax[s], q != jgw::kNone, q != jgw::kNone ? sc.uax[q] - sc.uax[s] : 0);
        const unsigned long long w = atomicAdd(cn + cCursor, 1ull);
        if (w >= cap) { atomicOr(cn + cErr, 2ull); continue; }
        out[w] = Tomb{k2[p], lo[i], hi[i], (uint32_t)(rbase[ir] + at), 0u};
    }
}
// The stored tags of U0, in (key, ord, tag) order, are tombstoned by the first Remove of the key's epoch-0 segment.
__global__ __launch_bounds__(kWB) void k_emit_u0(const Item* __restrict__ it, uint64_t T, const unsigned long long* __restrict__ k2,
                                                 const uint32_t* __restrict__ p2, const uint32_t* __restrict__ fr, const uint32_t* __restrict__ u0x,
                                                 const uint8_t* __restrict__ keep, const unsigned long long* __restrict__ rbase, uint64_t cap,
                                                 Tomb* __restrict__ out, unsigned long long* __restrict__ cn) {
    JGW_EACH(x, T) {
        const Item t = it[x];
        if (t.seg == jgw::kNone) continue;
        const uint32_t r = fr[t.seg];
        if (r == jgw::kNone) continue;
        const uint32_t ir = p2[r];
        if (!keep[ir]) continue;
        const unsigned long long w = atomicAdd(cn + cCursor, 1ull);
        if (w >= cap) { atomicOr(cn + cErr, 2ull); continue; }
        out[w] = Tomb{k2[t.seg], t.lo, t.hi, (uint32_t)(rbase[ir] + (x - u0x[t.seg])), 0u};
    }
}
__global__ __launch_bounds__(kWB) void k_split_tombs(const Tomb* __restrict__ in, uint64_t n, unsigned long long* __restrict__ key,
                                                     uint4* __restrict__ tag, uint32_t* __restrict__ ord) {
    JGW_EACH(x, n) {
        const Tomb t = in[x];
        key[x] = t.key;
        tag[x] = jgk::to_u4(Tag{t.lo, t.hi});
        ord[x] = t.ord;
    }
}
// The union's drop bitmap: one bit per Cleared set, `words` words.
__global__ __launch_bounds__(kWB) void k_drop_bits(const uint32_t* __restrict__ s1, const uint32_t* __restrict__ ss, const uint32_t* __restrict__ nclr,
                                                   uint64_t n, uint32_t words, unsigned* __restrict__ bits) {
    JGW_EACH(x, n) {
        if (ss[x] == x && nclr[x] > 0) {
            const uint32_t s = s1[x];
            if ((s >> 5) < words) atomicOr(bits + (s >> 5), 1u << (s & 31));
        }
    }
}

unsigned grid(jg_ctx* ctx, uint64_t n) { return jg::grid_for(ctx, n, kWB, 16); }

}  // namespace

namespace jg {

int orset_walk_default() {
    static const int mode = [] {
        const char* e = std::getenv("JANUS_ORSET_WALK");
        if (e && !std::strcmp(e, "host")) return 0;
        if (e && !std::strcmp(e, "device")) return 1;
        return 2;
    }();
    return mode;
}

void orset_walk_device(jg_orset* s, uint64_t n, const uint32_t* set, const uint32_t* elem, const uint8_t* op, const uint64_t* tag_lo,
                       const uint64_t* tag_hi, uint8_t* result, uint64_t* add_lim, uint64_t* rem_lim) {
    static const bool tr = std::getenv("JANUS_TRACE_APPLY") != nullptr;
    jg_ctx* ctx = s->ctx;
    hipStream_t st = ctx->stream;
    const int items = cub_count(n + 1, "ops");  // positions are 32-bit, marks 2p + 1
    JG_REQUIRE(n < 0x7FFFFFF0ull, JG_EINVAL, "jg_orset_apply_ops: %llu ops exceed one call", (unsigned long long)n);
    const int ni = items - 1;

    // phases on events, under the flag only
    constexpr int kEv = 8;
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

    // ---- the block ----
    uint32_t *d_set, *d_elem, *idx0, *p1, *s1, *p2, *t0, *t1, *t2, *t3, *t4, *x0, *x1, *x2, *x3, *x4, *ss, *epoch, *nclr, *e2, *seg, *kseg, *kf, *fr,
        *u0n, *u0x;
    uint8_t *d_op, *keep, *first, *cls, *issue_w, *d_res;
    unsigned long long *d_lo, *d_hi, *key, *k2, *bnd, *len, *ioff, *cnt_r, *va, *vr, *ax, *rx, *alim, *rlim, *abase, *rbase, *cn;
    TagRec* ts;
    Layout A, B;
    A.add(cn, cCount), A.add(d_set, n), A.add(d_elem, n), A.add(d_op, n), A.add(d_lo, n), A.add(d_hi, n), A.add(idx0, n), A.add(p1, n), A.add(s1, n);
    A.add(p2, n), A.add(key, n), A.add(k2, n), A.add(t0, n), A.add(t1, n), A.add(t2, n), A.add(t3, n), A.add(t4, n), A.add(x0, n), A.add(x1, n);
    A.add(x2, n), A.add(x3, n), A.add(x4, n), A.add(ss, n), A.add(epoch, n), A.add(nclr, n), A.add(e2, n), A.add(seg, n), A.add(kseg, n);
    A.add(kf, n), A.add(fr, n), A.add(u0n, n), A.add(u0x, n);
    B.add(keep, n), B.add(first, n), B.add(cls, n), B.add(issue_w, n), B.add(d_res, n), B.add(ts, n), B.add(bnd, 4 * n), B.add(len, n + 1);
    B.add(ioff, n + 1), B.add(cnt_r, n), B.add(va, n), B.add(vr, n), B.add(ax, n), B.add(rx, n), B.add(alim, n), B.add(rlim, n), B.add(abase, n);
    B.add(rbase, n);
    ensure(s->walk_ws, A.bytes() + B.bytes());
    A.bind(s->walk_ws.p);
    B.bind(s->walk_ws.as<char>() + A.bytes());
    const auto tmp = cub_in(s->walk_tmp);
    const unsigned g = grid(ctx, n);

    mark();
    JG_HIP(hipMemsetAsync(cn, 0, cCount * 8, st));
    JG_HIP(hipMemsetAsync(nclr, 0, n * 4, st));
    JG_HIP(hipMemsetAsync(kf, 0, n * 4, st));
    JG_HIP(hipMemsetAsync(u0n, 0, n * 4, st));
    JG_HIP(hipMemsetAsync(fr, 0xFF, n * 4, st));
    JG_HIP(hipMemcpyAsync(d_set, set, n * 4, hipMemcpyHostToDevice, st));
    JG_HIP(hipMemcpyAsync(d_elem, elem, n * 4, hipMemcpyHostToDevice, st));
    JG_HIP(hipMemcpyAsync(d_op, op, n, hipMemcpyHostToDevice, st));
    JG_HIP(hipMemcpyAsync(d_lo, tag_lo, n * 8, hipMemcpyHostToDevice, st));
    JG_HIP(hipMemcpyAsync(d_hi, tag_hi, n * 8, hipMemcpyHostToDevice, st));
    mark();  // upload

    // ---- order ----
    hipLaunchKernelGGL(k_prep, dim3(g), dim3(kWB), 0, st, d_set, d_elem, n, key, idx0);
    cub_run(tmp, [&](void* t, size_t& b) { return hipcub::DeviceRadixSort::SortPairs(t, b, d_set, s1, idx0, p1, ni, 0, 32, st); });
    cub_run(tmp, [&](void* t, size_t& b) { return hipcub::DeviceRadixSort::SortPairs(t, b, key, k2, idx0, p2, ni, 0, 64, st); });
    uint32_t *clr = t0, *cx = x0;
    hipLaunchKernelGGL(k_ord1_flags, dim3(g), dim3(kWB), 0, st, s1, p1, d_op, n, clr, t1);
    cub_run(tmp, [&](void* t, size_t& b) { return hipcub::DeviceScan::ExclusiveSum(t, b, clr, cx, ni, st); });
    cub_run(tmp, [&](void* t, size_t& b) { return hipcub::DeviceScan::InclusiveScan(t, b, t1, ss, hipcub::Max(), ni, st); });
    hipLaunchKernelGGL(k_epoch, dim3(g), dim3(kWB), 0, st, p1, clr, cx, ss, n, epoch, nclr);
    hipLaunchKernelGGL(k_keep, dim3(g), dim3(kWB), 0, st, s1, p1, ss, nclr, epoch, d_op, key, d_lo, d_hi, n, keep, ts, cn);
    hipLaunchKernelGGL(k_ord2_flags, dim3(g), dim3(kWB), 0, st, k2, p2, epoch, n, e2, t0, t1);
    cub_run(tmp, [&](void* t, size_t& b) { return hipcub::DeviceScan::InclusiveScan(t, b, t0, seg, hipcub::Max(), ni, st); });
    cub_run(tmp, [&](void* t, size_t& b) { return hipcub::DeviceScan::InclusiveScan(t, b, t1, kseg, hipcub::Max(), ni, st); });
    JG_HIP(hipGetLastError());
    mark();  // order

    // ---- classify ----
    hipLaunchKernelGGL(k_key_flags, dim3(g), dim3(kWB), 0, st, p2, d_op, e2, kseg, n, kf, fr);
    cub_run(tmp, [&](void* t, size_t& b) { return hipcub::DeviceMergeSort::SortKeys(t, b, ts, ni, TagLess{}, st); });
    hipLaunchKernelGGL(k_first, dim3(g), dim3(kWB), 0, st, ts, n, first);
    const View va_ = orset_view(s->add), vr_ = orset_view(s->rem);
    hipLaunchKernelGGL(k_bounds, dim3(grid(ctx, n + 1)), dim3(kWB), 0, st, va_, vr_, k2, kseg, e2, kf, n, bnd, len);
    cub_run(tmp, [&](void* t, size_t& b) { return hipcub::DeviceScan::ExclusiveSum(t, b, len, ioff, items, st); });
    JG_HIP(hipGetLastError());
    pin_get(ctx, 0, ioff + n, 8);
    pin_sync(ctx);
    uint64_t T;
    std::memcpy(&T, pin_at(ctx, 0), 8);
    const int t_items = cub_count(T, "stored tags under the batch's Removes and reads");
    Item* it = nullptr;
    if (T) {
        Layout C;
        C.add(it, T);
        ensure(s->walk_ws2, C.bytes());
        C.bind(s->walk_ws2.p);
        hipLaunchKernelGGL(k_items, dim3(grid(ctx, T)), dim3(kWB), 0, st, va_, vr_, ioff, bnd, n, T, it, u0n);
        cub_run(tmp, [&](void* t, size_t& b) { return hipcub::DeviceMergeSort::SortKeys(t, b, it, t_items, ItemLess{}, st); });
    }
    cub_run(tmp, [&](void* t, size_t& b) { return hipcub::DeviceScan::ExclusiveSum(t, b, u0n, u0x, ni, st); });
    hipLaunchKernelGGL(k_classify, dim3(g), dim3(kWB), 0, st, va_, vr_, p2, d_op, d_lo, d_hi, e2, seg, kseg, kf, first, bnd, n, cls, issue_w, t0, t1, t2,
                       t3, t4);
    JG_HIP(hipGetLastError());
    mark();  // classify

    // ---- scans ----
    cub_run(tmp, [&](void* t, size_t& b) { return hipcub::DeviceScan::ExclusiveSum(t, b, t0, x0, ni, st); });
    cub_run(tmp, [&](void* t, size_t& b) { return hipcub::DeviceScan::ExclusiveSum(t, b, t1, x1, ni, st); });
    cub_run(tmp, [&](void* t, size_t& b) { return hipcub::DeviceScan::ExclusiveSum(t, b, t2, x2, ni, st); });
    cub_run(tmp, [&](void* t, size_t& b) { return hipcub::DeviceScan::InclusiveScan(t, b, t3, x3, hipcub::Max(), ni, st); });
    cub_run(tmp, [&](void* t, size_t& b) { return hipcub::DeviceScan::InclusiveScan(t, b, t4, x4, hipcub::Max(), ni, st); });
    const Scans sc{x0, x1, x2, x3, x4};
    hipLaunchKernelGGL(k_eval, dim3(g), dim3(kWB), 0, st, p2, d_op, d_elem, e2, seg, kseg, kf, bnd, u0n, sc, keep, n, d_res, cnt_r, cn);
    hipLaunchKernelGGL(k_ord1_counts, dim3(g), dim3(kWB), 0, st, p1, issue_w, cnt_r, n, va, vr);
    cub_run(tmp, [&](void* t, size_t& b) { return hipcub::DeviceScan::ExclusiveSum(t, b, va, ax, ni, st); });
    cub_run(tmp, [&](void* t, size_t& b) { return hipcub::DeviceScan::ExclusiveSum(t, b, vr, rx, ni, st); });
    hipLaunchKernelGGL(k_lims, dim3(g), dim3(kWB), 0, st, p1, va, vr, ax, rx, keep, n, alim, rlim, abase, rbase, cn);
    uint32_t *ka = t0, *kax = t1;  // (the flags' inputs are spent; their sums x0..x4 live on)
    hipLaunchKernelGGL(k_add_flags, dim3(g), dim3(kWB), 0, st, ts, issue_w, keep, n, ka);
    cub_run(tmp, [&](void* t, size_t& b) { return hipcub::DeviceScan::ExclusiveSum(t, b, ka, kax, ni, st); });
    JG_HIP(hipGetLastError());
    pin_get(ctx, 0, cn, cCount * 8);
    pin_get(ctx, 256, kax + (n - 1), 4);
    pin_get(ctx, 260, ka + (n - 1), 4);
    pin_sync(ctx);
    mark();  // scans
    unsigned long long h[cCount];
    uint32_t last[2];
    std::memcpy(h, pin_at(ctx, 0), sizeof h);
    std::memcpy(last, pin_at(ctx, 256), sizeof last);
    const uint64_t n_add = (uint64_t)last[0] + last[1], n_rem = h[cKeptR];

    s->walk_stats[0] += 1;
    s->walk_stats[2] += n;
    auto copy_out = [&](uint64_t base_a, uint64_t base_r) {
        JG_HIP(hipMemcpyAsync(result, d_res, n, hipMemcpyDeviceToHost, st));
        if (add_lim) {
            JG_HIP(hipMemcpyAsync(add_lim, alim, n * 8, hipMemcpyDeviceToHost, st));
            JG_HIP(hipMemcpyAsync(rem_lim, rlim, n * 8, hipMemcpyDeviceToHost, st));
        }
        JG_HIP(hipStreamSynchronize(st));
        if (add_lim)
            for (uint64_t i = 0; i < n; ++i) add_lim[i] += base_a, rem_lim[i] += base_r;
    };
    if (n_add == 0 && n_rem == 0 && h[cCleared] == 0) {
        copy_out(s->add.next, s->rem.next);
        return;
    }
    JG_REQUIRE(h[cNextA] < 0xFFFFFFFFull && h[cNextR] < 0xFFFFFFFFull, JG_EINVAL, "jg_orset_apply_ops: too many records in one batch");

    // ---- emit ----
    jg_orset batch;
    batch.ctx = ctx;
    set_dense(ctx, batch.add, n_add);
    set_dense(ctx, batch.rem, n_rem);
    batch.add.next = h[cSpanA];
    batch.rem.next = h[cSpanR];
    if (n_add)
        hipLaunchKernelGGL(k_emit_add, dim3(g), dim3(kWB), 0, st, ts, ka, kax, abase, n, n_add, batch.add.key.as<unsigned long long>(),
                           batch.add.tag.as<uint4>(), batch.add.ord.as<uint32_t>(), cn);
    if (n_rem) {
        Tomb* tb;
        Layout D;
        D.add(tb, n_rem);
        ensure(s->walk_ws3, D.bytes());
        D.bind(s->walk_ws3.p);
        hipLaunchKernelGGL(k_emit_uadd, dim3(g), dim3(kWB), 0, st, k2, p2, d_lo, d_hi, cls, e2, seg, kseg, kf, bnd, u0n, sc, keep, rbase, n, n_rem, tb, cn);
        if (T)
            hipLaunchKernelGGL(k_emit_u0, dim3(grid(ctx, T)), dim3(kWB), 0, st, it, T, k2, p2, fr, u0x, keep, rbase, n_rem, tb, cn);
        const int r_items = cub_count(n_rem, "tombstones");
        cub_run(tmp, [&](void* t, size_t& b) { return hipcub::DeviceMergeSort::SortKeys(t, b, tb, r_items, TombLess{}, st); });
        hipLaunchKernelGGL(k_split_tombs, dim3(grid(ctx, n_rem)), dim3(kWB), 0, st, tb, n_rem, batch.rem.key.as<unsigned long long>(),
                           batch.rem.tag.as<uint4>(), batch.rem.ord.as<uint32_t>());
    }
    DevBuf drop;
    jgk::Drop d{nullptr, 0};
    if (h[cCleared]) {
        const uint32_t words = (uint32_t)(h[cMaxCleared] >> 5) + 1;
        drop.alloc((size_t)words * 4);
        JG_HIP(hipMemsetAsync(drop.p, 0, (size_t)words * 4, st));
        hipLaunchKernelGGL(k_drop_bits, dim3(g), dim3(kWB), 0, st, s1, ss, nclr, n, words, drop.as<unsigned>());
        d = jgk::Drop{drop.as<unsigned>(), words};
    }
    JG_HIP(hipGetLastError());
    // the emitted counts against the counted ones, before anything reaches the store
    pin_get(ctx, 0, cn, cCount * 8);
    pin_sync(ctx);
    std::memcpy(h, pin_at(ctx, 0), sizeof h);
    JG_REQUIRE(h[cErr] == 0 && h[cCursor] == n_rem, JG_ESTATE, "jg_orset_apply_ops: the device walk emitted %llu tombstones for %llu counted (flag %llu)",
               h[cCursor], (unsigned long long)n_rem, h[cErr]);
    mark();  // emit

    // ---- union ----
    uint64_t base_a = 0, base_r = 0;
    orset_walk_union(s, &batch, d, &base_a, &base_r);
    mark();  // union
    copy_out(base_a, base_r);
    mark();  // copies out
    if (tr && n_ev == kEv) {
        float ms[kEv - 1];
        JG_HIP(hipEventSynchronize(ev[kEv - 1]));
        for (int i = 0; i + 1 < kEv; ++i) JG_HIP(hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
        std::fprintf(stderr, "orset apply_ops on the device (%llu ops, %llu+%llu records, %llu stored tags read): upload %.2f ms, order %.2f ms, "
                     "classify %.2f ms, scans %.2f ms, emit %.2f ms, union %.2f ms, copies out %.2f ms\n", (unsigned long long)n,
                     (unsigned long long)n_add, (unsigned long long)n_rem, (unsigned long long)T, ms[0], ms[1], ms[2], ms[3], ms[4], ms[5], ms[6]);
    }
}

}  // namespace jg

extern "C" {

int jg_orset_set_walk(jg_orset* s, int mode) {
    return jg::guard([&] {
        auto lk_ = jg::lock(s);
        JG_REQUIRE(s, JG_EINVAL, "jg_orset_set_walk: store is NULL");
        JG_REQUIRE(mode >= 0 && mode <= 2, JG_EINVAL, "jg_orset_set_walk: mode %d is not 0 (host), 1 (device) or 2 (auto)", mode);
        s->walk_mode = mode;
    });
}

int jg_orset_walk_stats(jg_orset* s, uint64_t out[4]) {
    return jg::guard([&] {
        auto lk_ = jg::lock(s);
        JG_REQUIRE(s && out, JG_EINVAL, "jg_orset_walk_stats: NULL argument");
        for (int i = 0; i < 4; ++i) out[i] = s->walk_stats[i];
    });
}

}  // extern "C"
