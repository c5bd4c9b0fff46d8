// orset_names.hip — the OR-Set by element name: Contains, LookupAll and Add / Remove / Clear over strings, resolved
// and interned in the store's own element table (orset_names.hpp).
//
// The reference's ORSet<string> takes strings everywhere (MergeSharp/MergeSharp/CRDTs/ORSet.cs:134-237); the store's
// records are (set << 32 | element id, tag).  The element table that wave commits and jg_orset_names_sync fill
// already maps (set, string) -> id on the device; these entry points ask it, and intern into it outside a wave:
//
//   resolve   k_nm_resolve, one lane per name: FNV-1a -> name_key & kmask -> tab_find.  jg_orset_resolve_names
//             copies the ids out; jg_orset_contains_names writes set << 32 | id into the query array that
//             jg_orset_contains' kernel reads from device memory (no id round trip).
//   lookup    jg_orset_lookup_all's two passes into device scratch, k_nm_lens (itab_find per member), a device
//             scan for name_off, k_nm_copy (one lane per output byte), one D2H per output array.
//   intern    jg_orset_apply_ops_names.  Every op carries its Clear epoch (Clears of its set before it, counted on
//             the host); the resident table answers for epoch 0 only.
//             k_nm_claim   Adds whose name is not live enter a call-wide open-addressing table keyed by (set, epoch,
//                          name): a slot is claimed by CAS with the claimant's op index, a tag match is confirmed
//                          against the claimant's bytes in the uploaded op buffer (immutable input), a lost CAS is
//                          answered by the value it returned, and atomicMin behind a plain read keeps the first
//                          Add's op index per name.  No lane waits for another.
//             k_nm_win     (next launch) the first Add of each new name is a winner: its log position and pool
//                          offset come from two scans in op order, its id from a sort by (set, op index):
//                          k_nm_assign gives next_id[set] + rank.
//             k_nm_ids     every op's id: the resident id, or the new name's id from its first Add onward, else
//                          JG_NULL_ELEM - 1.  The ids (4 B per op) go to the host for the record side
//                          (jg_orset_apply_ops' walk and union), which runs BEFORE the table changes.
//                          Op 4 (internal: a read inside a batch, jg_node_exec_keys) is resolved as a Remove: it
//                          claims nothing and interns nothing.
//             k_nm_put     appends the winners to the names log with gen = set_gen[set] + epoch; k_nm_sets then
//                          advances next_id and set_gen.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "launch.hpp"
#include "orset_layouts.hpp"
#include "orset_names.hpp"

namespace {

using namespace jgn;

constexpr int kBlock = 256;
constexpr uint32_t kNever = JG_NULL_ELEM - 1;  // "never allocated": the id no record carries
constexpr uint32_t kMaxSet = 0xFFFFFFF0u;      // set ids stay below it (as jg_orset_wave_append)
constexpr unsigned long long kNoWin = ~0ull;

using jg::blocks_for;

// The uploaded name arrays (one staging copy): meta = is_null | op << 1 (op 0 for the read-only calls).
struct Staged {
    const uint64_t* off;
    const uint32_t* set;
    const uint32_t* epoch;  // apply_ops_names only
    const uint8_t* meta;
    const uint8_t* bytes;
};

__device__ __forceinline__ uint64_t fnv_of(const uint8_t* b, uint32_t len) {
    uint64_t h = kFnvBasis;
    for (uint32_t k = 0; k < len; ++k) h = (h ^ b[k]) * kFnvPrime;
    return h;
}

// ---- resolve (read-only) -------------------------------------------------------------------------------
__global__ void k_nm_resolve(Names N, uint64_t set_cap, uint64_t kmask, uint64_t salt, Staged S, uint64_t n, uint32_t* __restrict__ elem,
                             unsigned long long* __restrict__ q) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t set = S.set[i];
    uint32_t id = JG_NULL_ELEM;
    if (!(S.meta[i] & 1)) {
        id = kNoName;
        if (set < set_cap) {  // a set the table never saw has no names
            const uint8_t* b = S.bytes + S.off[i];
            const uint32_t len = (uint32_t)(S.off[i + 1] - S.off[i]);
            id = tab_find(N, name_key(set, fnv_of(b, len), salt) & kmask, set, b, len);
        }
        if (id == kNoName) id = kNever;
    }
    if (elem) elem[i] = id;
    if (q) q[i] = (unsigned long long)set << 32 | id;
}

// ---- lookup_all by name --------------------------------------------------------------------------------
__global__ void k_nm_lens(Names N, const uint64_t* __restrict__ moff, uint64_t n_sets, const uint32_t* __restrict__ sets,
                          const uint32_t* __restrict__ elems, uint64_t total, uint32_t* __restrict__ g_of, unsigned long long* __restrict__ len,
                          uint8_t* __restrict__ is_null, unsigned long long* __restrict__ missing) {
    const uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= total) return;
    const uint32_t id = elems[k];
    uint32_t g = kNoName;
    if (id != JG_NULL_ELEM) {
        uint64_t lo = 0, hi = n_sets;  // the member's set: the last query whose offset is <= k
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (moff[mid] <= k) lo = mid;
            else hi = mid;
        }
        g = itab_find(N, sets[lo], id);
        if (g == kNoName) *missing = 1;
    }
    g_of[k] = g;
    len[k] = g == kNoName ? 0ull : (unsigned long long)N.len[g];
    is_null[k] = id == JG_NULL_ELEM ? 1 : 0;
}

// One lane per output byte: its member by a search of name_off (coalesced stores).
__global__ void k_nm_copy(Names N, const unsigned long long* __restrict__ name_off, const uint32_t* __restrict__ g_of, uint64_t total,
                          uint64_t n_bytes, uint8_t* __restrict__ out) {
    const uint64_t b = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= n_bytes) return;
    uint64_t lo = 0, hi = total;  // the last member whose offset is <= b (empty names share an offset with their successor)
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (name_off[mid] <= b) lo = mid;
        else hi = mid;
    }
    out[b] = N.pool[N.off[g_of[lo]] + (b - name_off[lo])];
}

// ---- interning (apply_ops_names) -----------------------------------------------------------------------
// The call's table of new names: slot word = tag << 32 | claimant's op index + 1 (0 = empty); first[slot] = the
// smallest op index of an Add of that name.
struct Cand {
    unsigned long long* slot;
    uint32_t* first;
    uint64_t mask;
};

__device__ __forceinline__ uint64_t cand_key(uint64_t nkey, uint32_t epoch) { return mix64(nkey + (uint64_t)epoch * 0x9E3779B97F4A7C15ull + 1); }

__device__ __forceinline__ bool cand_same(const Staged& S, uint32_t j, uint32_t set, uint32_t epoch, const uint8_t* b, uint32_t len) {
    return S.set[j] == set && S.epoch[j] == epoch && (uint32_t)(S.off[j + 1] - S.off[j]) == len && same_bytes(S.bytes + S.off[j], b, len);
}

// The slot of (set, epoch, name), claimed for op i if absent (claim) or kNoName if absent (!claim).
template <bool CLAIM>
__device__ __forceinline__ uint32_t cand_probe(const Cand& C, const Staged& S, uint64_t ck, uint32_t i, uint32_t set, uint32_t epoch,
                                               const uint8_t* b, uint32_t len) {
    const unsigned long long mine = (ck >> 32) << 32 | (unsigned long long)(i + 1);
    for (uint64_t s = ck & C.mask;; s = (s + 1) & C.mask) {
        unsigned long long w = C.slot[s];
        if (w == 0) {
            if (!CLAIM) return kNoName;
            w = atomicCAS(C.slot + s, 0ull, mine);
            if (w == 0) return (uint32_t)s;  // claimed; a lost CAS is answered by the word it returned
        }
        if ((w >> 32) == (mine >> 32) && cand_same(S, (uint32_t)w - 1, set, epoch, b, len)) return (uint32_t)s;
    }
}

// rid[i]: the resident id (epoch 0 only) or kNoName; nkey[i]: the name key; Adds of names that are not live claim.
__global__ void k_nm_claim(Names N, uint64_t kmask, uint64_t salt, Staged S, uint64_t n, Cand C, uint32_t* __restrict__ rid,
                           unsigned long long* __restrict__ nkey, uint32_t* __restrict__ slot) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t m = S.meta[i], op = m >> 1;
    uint32_t id = kNoName, sl = kNoName;
    unsigned long long key = 0;
    if (op != 3 && !(m & 1)) {
        const uint32_t set = S.set[i], epoch = S.epoch[i];
        const uint8_t* b = S.bytes + S.off[i];
        const uint32_t len = (uint32_t)(S.off[i + 1] - S.off[i]);
        key = name_key(set, fnv_of(b, len), salt) & kmask;
        if (epoch == 0) id = tab_find(N, key, set, b, len);  // after a Clear in the batch the resident names are dead
        if (id == kNoName && op == 1) {
            sl = cand_probe<true>(C, S, cand_key(key, epoch), (uint32_t)i, set, epoch, b, len);
            if (C.first[sl] > (uint32_t)i) atomicMin(C.first + sl, (uint32_t)i);  // a plain read first: 64 Adds of one name
        }
    }
    rid[i] = id;
    nkey[i] = key;
    slot[i] = sl;
}

// The first Add of each new name wins: one log entry (cnt), its bytes (len), its sort key (set << 32 | op index).
__global__ void k_nm_win(Staged S, uint64_t n, Cand C, const uint32_t* __restrict__ slot, unsigned long long* __restrict__ cnt,
                         unsigned long long* __restrict__ len, unsigned long long* __restrict__ wkey) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i > n) return;
    bool win = false;
    if (i < n) {
        const uint32_t sl = slot[i];
        win = sl != kNoName && C.first[sl] == (uint32_t)i;
    }
    cnt[i] = win ? 1ull : 0ull;  // [n] = 0: the exclusive scans leave the totals there
    len[i] = win ? (unsigned long long)(S.off[i + 1] - S.off[i]) : 0ull;
    if (i < n) wkey[i] = win ? (unsigned long long)S.set[i] << 32 | i : kNoWin;
}

__device__ __forceinline__ uint64_t set_begin(const unsigned long long* k, uint64_t n, uint32_t set) {
    uint64_t lo = 0, hi = n;
    const unsigned long long x = (unsigned long long)set << 32;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (k[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Winners sorted by (set, op index): the r-th of a set takes next_id + r.  st[0]: a set out of ids, st[1]: max id + 1.
__global__ void k_nm_assign(Names N, const unsigned long long* __restrict__ skey, uint64_t n, uint32_t* __restrict__ newid,
                            unsigned long long* __restrict__ st) {
    const uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= n || skey[k] == kNoWin) return;
    const uint32_t set = (uint32_t)(skey[k] >> 32), i = (uint32_t)skey[k];
    const uint64_t id = (uint64_t)N.next_id[set] + (k - set_begin(skey, n, set));
    if (id >= kNever) atomicOr(st, 1ull);
    newid[i] = (uint32_t)id;
    atomicMax(st + 1, (unsigned long long)id + 1);
}

__global__ void k_nm_ids(Staged S, uint64_t n, Cand C, const uint32_t* __restrict__ rid, const unsigned long long* __restrict__ nkey,
                         const uint32_t* __restrict__ slot, const uint32_t* __restrict__ newid, uint32_t* __restrict__ elem) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t m = S.meta[i], op = m >> 1;
    uint32_t id;
    if (op == 3) id = 0;
    else if (m & 1) id = JG_NULL_ELEM;
    else if (rid[i] != kNoName) id = rid[i];
    else if (op == 1) id = newid[C.first[slot[i]]];
    else {  // Remove: live only if this batch interned the name, in this epoch, at an earlier op
        const uint32_t set = S.set[i], epoch = S.epoch[i];
        const uint32_t sl = cand_probe<false>(C, S, cand_key(nkey[i], epoch), (uint32_t)i, set, epoch, S.bytes + S.off[i],
                                              (uint32_t)(S.off[i + 1] - S.off[i]));
        id = sl != kNoName && C.first[sl] < (uint32_t)i ? newid[C.first[sl]] : kNever;
    }
    elem[i] = id;
}

// Winners appended to the names log in op order (pos / poff: the scans of k_nm_win's cnt / len).
__global__ void k_nm_put(Names N, uint64_t g0, uint64_t pool0, Staged S, uint64_t n, const unsigned long long* __restrict__ pos,
                         const unsigned long long* __restrict__ poff, const unsigned long long* __restrict__ nkey,
                         const uint32_t* __restrict__ newid) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || pos[i + 1] == pos[i]) return;
    const uint64_t g = g0 + pos[i], p = pool0 + poff[i];
    const uint32_t set = S.set[i], len = (uint32_t)(S.off[i + 1] - S.off[i]), id = newid[i];
    const uint8_t* src = S.bytes + S.off[i];
    for (uint32_t k = 0; k < len; ++k) N.pool[p + k] = src[k];
    N.set[g] = set;
    N.id[g] = id;
    N.gen[g] = N.set_gen[set] + S.epoch[i];
    N.len[g] = len;
    N.off[g] = p;
    N.key[g] = nkey[i];
    tab_insert(N, nkey[i], (uint32_t)g);
    itab_insert(N, set, id, (uint32_t)g);
}

// After the put: next_id past each set's new names (the set's last winner adds its count), set_gen past its Clears.
__global__ void k_nm_sets(Names N, const unsigned long long* __restrict__ skey, uint64_t n, const uint32_t* __restrict__ cset,
                          const uint32_t* __restrict__ ccnt, uint64_t n_cleared) {
    const uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k < n_cleared) N.set_gen[cset[k]] += ccnt[k];
    if (k >= n || skey[k] == kNoWin) return;
    const uint32_t set = (uint32_t)(skey[k] >> 32);
    if (k + 1 < n && skey[k + 1] != kNoWin && (uint32_t)(skey[k + 1] >> 32) == set) return;  // not the set's last winner
    N.next_id[set] += (uint32_t)(k + 1 - set_begin(skey, n, set));
}

// ---- host side -----------------------------------------------------------------------------------------
// Argument checks of a name array (before anything changes); returns the largest set id + 1.
uint64_t check_names(const char* fn, uint64_t n, const uint32_t* set, const uint64_t* off, const uint8_t* bytes, const uint8_t* is_null) {
    JG_REQUIRE(set && off && is_null, JG_EINVAL, "%s: NULL argument", fn);
    JG_REQUIRE(off[0] == 0, JG_EINVAL, "%s: off[0] must be 0", fn);
    uint64_t mx = 0;
    for (uint64_t i = 0; i < n; ++i) {
        JG_REQUIRE(off[i + 1] >= off[i] && off[i + 1] - off[i] < 0x7FFFFFFFull, JG_EINVAL, "%s: bad offsets at name %llu", fn, (unsigned long long)i);
        JG_REQUIRE(set[i] < kMaxSet, JG_EINVAL, "%s: set id %u out of range", fn, set[i]);
        mx = std::max<uint64_t>(mx, (uint64_t)set[i] + 1);
    }
    JG_REQUIRE(bytes || off[n] == 0, JG_EINVAL, "%s: NULL argument", fn);
    return mx;
}

// The name arrays packed for one copy: off [n + 1] u64 | set [n] u32 | epoch [n] u32 | cset, ccnt [nc] u32 | meta [n] | bytes.
struct Packed {
    std::vector<uint8_t> h;
    size_t at_set, at_epoch, at_cset, at_ccnt, at_meta, at_bytes;
    Packed(uint64_t n, uint64_t nc, const uint32_t* set, const uint64_t* off, const uint8_t* bytes) {
        at_set = (n + 1) * 8;
        at_epoch = at_set + n * 4;
        at_cset = at_epoch + n * 4;
        at_ccnt = at_cset + nc * 4;
        at_meta = at_ccnt + nc * 4;
        at_bytes = jg::round_up(at_meta + n, 8);
        h.resize(at_bytes + off[n]);
        std::memcpy(h.data(), off, (n + 1) * 8);
        std::memcpy(h.data() + at_set, set, n * 4);
        if (off[n]) std::memcpy(h.data() + at_bytes, bytes, off[n]);
    }
    uint32_t* epoch() { return reinterpret_cast<uint32_t*>(h.data() + at_epoch); }
    uint32_t* cset() { return reinterpret_cast<uint32_t*>(h.data() + at_cset); }
    uint32_t* ccnt() { return reinterpret_cast<uint32_t*>(h.data() + at_ccnt); }
    uint8_t* meta() { return h.data() + at_meta; }
    Staged on(const uint8_t* d) const {
        return Staged{reinterpret_cast<const uint64_t*>(d), reinterpret_cast<const uint32_t*>(d + at_set),
                      reinterpret_cast<const uint32_t*>(d + at_epoch), d + at_meta, d + at_bytes};
    }
};

// Resolve n names into device ids and / or query keys: the staging and both outputs in ctx->scratch.
struct Resolved {
    uint32_t* elem;
    unsigned long long* q;
    uint8_t* out;  // n bytes behind them (contains' answers)
};
Resolved resolve_on_device(jg_orset* s, Packed& P, uint64_t n, const uint8_t* is_null) {
    jg_ctx* ctx = s->ctx;
    std::memset(P.epoch(), 0, n * 4);
    for (uint64_t i = 0; i < n; ++i) P.meta()[i] = is_null[i] ? 1 : 0;
    jg::ElemTable& T = *jg::orset_elem_table(s, true);
    T.ensure_names(ctx, 0, 0);
    Resolved r{};
    uint8_t* d;  // the staged arrays, at the block's start
    jg::Layout L;
    L.add(d, P.h.size(), 8), L.add(r.q, n, 8), L.add(r.elem, n, 8), L.add(r.out, n, 8);
    L.bind(jg::scratch(ctx, ctx->scratch, L.bytes() + 64));
    JG_HIP(hipMemcpyAsync(d, P.h.data(), P.h.size(), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_nm_resolve, dim3(blocks_for(n)), dim3(kBlock), 0, ctx->stream, T.view(), T.set_cap, T.kmask, T.salt, P.on(d), n, r.elem, r.q);
    JG_HIP(hipGetLastError());
    return r;
}

void scan_in_place(jg_ctx* ctx, unsigned long long* d, uint64_t n) {
    const int items = jg::cub_count(n);
    jg::cub_run(jg::cub_in(ctx, ctx->scratch3),
                [&](void* temp, size_t& bytes) { return hipcub::DeviceScan::ExclusiveSum(temp, bytes, d, d, items, ctx->stream); });
}

// ---- the table itself (jg::ElemTable): rebuilds after growth, jg_orset_names_sync's updates ---------------------
__global__ void k_names_rebuild(Names N, uint64_t n_names) {
    const uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g < n_names && N.gen[g] == N.set_gen[N.set[g]]) tab_insert(N, N.key[g], (uint32_t)g);
}

__global__ void k_itab_rebuild(Names N, uint64_t n_names) {
    const uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g < n_names) itab_insert(N, N.set[g], N.id[g], (uint32_t)g);
}

__global__ void k_sets_update(Names N, const uint32_t* __restrict__ set, const uint32_t* __restrict__ next, const uint8_t* __restrict__ cleared, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    if (cleared[i]) N.set_gen[set[i]] += 1;
    N.next_id[set[i]] = next[i];
}

__global__ void k_names_put(Names N, uint64_t g0, uint64_t pool0, const uint32_t* __restrict__ nset, const uint32_t* __restrict__ nid,
                            const uint64_t* __restrict__ off, uint64_t n, uint64_t kmask, uint64_t salt) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t g = g0 + i;
    const uint32_t set = nset[i], len = (uint32_t)(off[i + 1] - off[i]);
    const uint8_t* b = N.pool + pool0 + off[i];
    uint64_t h = kFnvBasis;
    for (uint32_t k = 0; k < len; ++k) h = (h ^ b[k]) * kFnvPrime;
    const uint64_t key = name_key(set, h, salt) & kmask;
    N.set[g] = set;
    N.id[g] = nid[i];
    N.gen[g] = N.set_gen[set];
    N.len[g] = len;
    N.off[g] = pool0 + off[i];
    N.key[g] = key;
    tab_insert(N, key, (uint32_t)g);
    itab_insert(N, set, nid[i], (uint32_t)g);
}

// The page-locked staging (layout: jg::NamesStaging, orset_layouts.hpp) with room for `need` bytes.
void names_reserve(jg::ElemTable::NamesOut& o, size_t need) {
    if (o.cap >= need) return;
    if (o.ev) JG_HIP(hipEventSynchronize(o.ev));  // no earlier copy may still land in the old block
    if (o.host) JG_HIP(hipHostFree(o.host));
    o.host = nullptr;
    o.cap = 0;
    void* p = nullptr;
    JG_HIP(hipHostMalloc(&p, need + need / 2, hipHostMallocDefault));
    o.host = static_cast<uint8_t*>(p);
    o.cap = need + need / 2;
}

// The copies of L.n names from `from` on and the nb pool bytes from pool0 on into the staging, queued on q.
void names_stage(jg::ElemTable& T, const jg::NamesStaging& L, uint64_t from, uint64_t pool0, uint64_t nb, hipStream_t q) {
    uint8_t* h = T.nout.host;
    JG_HIP(hipMemcpyAsync(h + L.set, T.nset.as<uint32_t>() + from, L.n * 4, hipMemcpyDeviceToHost, q));
    JG_HIP(hipMemcpyAsync(h + L.id, T.nid.as<uint32_t>() + from, L.n * 4, hipMemcpyDeviceToHost, q));
    JG_HIP(hipMemcpyAsync(h + L.len, T.nlen.as<uint32_t>() + from, L.n * 4, hipMemcpyDeviceToHost, q));
    JG_HIP(hipMemcpyAsync(h + L.pool_off, T.noff.as<unsigned long long>() + from, L.n * 8, hipMemcpyDeviceToHost, q));
    if (nb) JG_HIP(hipMemcpyAsync(h + L.pool, T.pool.as<uint8_t>() + pool0, nb, hipMemcpyDeviceToHost, q));
}

// Names [from, to), whose bytes lie in the pool range [pool0, pool1), in the staging as a pull (a queued wave-names
// copy is gone): staged on ctx->stream and waited for, unless the staging holds exactly that pull already.
void names_stage_now(jg_ctx* ctx, jg::ElemTable& T, uint64_t from, uint64_t to, uint64_t pool0, uint64_t pool1, const char* who) {
    auto& o = T.nout;
    if (o.since_from == from && o.since_to == to && o.since_pool0 == pool0 && o.since_pool1 == pool1) return;
    const jg::NamesStaging L(to - from, pool1 - pool0);
    if (o.ev) JG_HIP(hipEventSynchronize(o.ev));
    o.g0 = o.g1 = 0;
    names_reserve(o, L.bytes);
    names_stage(T, L, from, pool0, pool1 - pool0, ctx->stream);
    JG_HIP(hipStreamSynchronize(ctx->stream));
    const auto* hlen = reinterpret_cast<const uint32_t*>(o.host + L.len);
    const auto* hat = reinterpret_cast<const uint64_t*>(o.host + L.pool_off);
    uint64_t sum = 0;
    for (uint64_t i = 0; i < L.n; ++i) {
        const uint64_t at = hat[i], len = hlen[i];
        JG_REQUIRE(at >= pool0 && at + len <= pool1, JG_ESTATE, "%s: name %llu's bytes lie outside the pool range of its log position", who,
                   (unsigned long long)(from + i));
        sum += len;
    }
    o.since_from = from, o.since_to = to, o.since_pool0 = pool0, o.since_pool1 = pool1, o.since_bytes = sum;
}

// Queue the copy of the names [g0, g1) / pool bytes [p0, p1) the last commit issued (async on ctx->stream).
void queue_names(jg_ctx* ctx, jg::ElemTable& T) {
    auto& o = T.nout;
    o.g0 = o.g1 = 0;
    o.since_from = UINT64_MAX;  // the staging is about to hold this commit's names
    const uint64_t n = T.g1 - T.g0, nb = T.p1 - T.p0;
    if (n == 0) return;
    const jg::NamesStaging L(n, nb);
    names_reserve(o, L.bytes);
    if (!o.ev) JG_HIP(hipEventCreateWithFlags(&o.ev, hipEventDisableTiming));
    // on the copy queue (idle once a wave's uploads are in), behind the commit's kernels: the record sorts and
    // the union behind them on ctx->stream do not wait for these copies.  The names arrays are only ever
    // appended to past g1 / p1 or reallocated, and a reallocation (grow_keep) syncs the copy queue first.
    hipStream_t q = ctx->copy ? ctx->copy : ctx->stream;
    if (q != ctx->stream) {
        JG_HIP(hipEventRecord(o.ev, ctx->stream));
        JG_HIP(hipStreamWaitEvent(q, o.ev, 0));
    }
    names_stage(T, L, T.g0, T.p0, nb, q);
    JG_HIP(hipEventRecord(o.ev, q));
    o.g0 = T.g0, o.g1 = T.g1, o.p0 = T.p0, o.p1 = T.p1;
}

}  // namespace

namespace jg {

ElemTable::~ElemTable() {
    for (void* p : retired) (void)hipFree(p);
    if (nout.ev) (void)hipEventSynchronize(nout.ev);
    if (nout.host) (void)hipHostFree(nout.host);
    if (nout.ev) (void)hipEventDestroy(nout.ev);
}

Names ElemTable::view() const {
    return Names{tab.as<unsigned long long>(), tab_cap ? tab_cap - 1 : 0, nset.as<uint32_t>(), nid.as<uint32_t>(), ngen.as<uint32_t>(), nlen.as<uint32_t>(),
                 noff.as<unsigned long long>(), nkey.as<unsigned long long>(), pool.as<uint8_t>(), set_gen.as<uint32_t>(), next_id.as<uint32_t>(),
                 ikey.as<unsigned long long>(), ival.as<uint32_t>(), itab_cap ? itab_cap - 1 : 0};
}

void ElemTable::ensure_sets(jg_ctx* ctx, uint64_t n_sets) {
    if (n_sets <= set_cap) return;
    const uint64_t cap = std::max<uint64_t>(n_sets + n_sets / 2, 1024);
    grow_keep(ctx, set_gen, cap * 4, set_cap * 4, true, &retired);
    grow_keep(ctx, next_id, cap * 4, set_cap * 4, true, &retired);
    set_cap = set_gen.bytes / 4;
}

void ElemTable::ensure_names(jg_ctx* ctx, uint64_t incoming, uint64_t pool_bytes) {
    const uint64_t total = n_names + incoming;
    JG_REQUIRE(total < 0xFFFFFFF0ull, JG_ESTATE, "OR-Set element table: more than 2^32 names");
    if (total > name_cap) {
        const uint64_t cap = std::max<uint64_t>(total + total / 2, 4096);
        // the per-name arrays: {buffer, element size}
        const std::pair<DevBuf*, size_t> arrays[] = {{&nset, 4}, {&nid, 4}, {&ngen, 4}, {&nlen, 4}, {&noff, 8}, {&nkey, 8}};
        for (const auto& [b, size] : arrays) grow_keep(ctx, *b, cap * size, n_names * size, false, &retired);
        name_cap = std::min({nset.bytes / 4, nid.bytes / 4, ngen.bytes / 4, nlen.bytes / 4, noff.bytes / 8, nkey.bytes / 8});
    }
    if (pool_used + pool_bytes > pool_cap) {  // x1.5: a pool grown to the exact need grew again every wave
        grow_keep(ctx, pool, std::max<uint64_t>({pool_used + pool_bytes, pool_cap + pool_cap / 2, 1 << 20}), pool_used, false, &retired);
        pool_cap = pool.bytes;
    }
    // a hash table outgrown: its block retired, not freed (see grow_keep), a new one zeroed and filled again
    const auto regrow = [&](DevBuf& b, size_t bytes, bool zero) {
        if (b.p) retired.push_back(b.p);
        b.p = nullptr;
        b.bytes = 0;
        b.alloc(bytes);
        if (zero) JG_HIP(hipMemsetAsync(b.p, 0, bytes, ctx->stream));
    };
    if (tab_cap == 0 || 2 * total > tab_cap) {
        tab_cap = pow2_at_least(4 * total, 1024);
        regrow(tab, tab_cap * 8, true);
        if (n_names) hipLaunchKernelGGL(k_names_rebuild, dim3(blocks_for(n_names)), dim3(kBlock), 0, ctx->stream, view(), n_names);
        JG_HIP(hipGetLastError());
    }
    if (itab_cap == 0 || 2 * total > itab_cap) {  // the (set, id) index: every name, load <= 1/2
        itab_cap = pow2_at_least(4 * total, 1024);
        regrow(ikey, itab_cap * 8, true);
        regrow(ival, itab_cap * 4, false);
        if (n_names) hipLaunchKernelGGL(k_itab_rebuild, dim3(blocks_for(n_names)), dim3(kBlock), 0, ctx->stream, view(), n_names);
        JG_HIP(hipGetLastError());
    }
}

// id_bound sums the names every commit issued over ALL sets, so on a store with many sets it grows far past any
// one set's next id and would refuse waves every set still has room for.  Before refusing, the
// bound is tightened to the exact largest per-set next id (one device max over the sets, one round trip); the
// check then asks whether that set plus every name of the wave could pass 2^32 - 2 — still conservative (all
// names counted against the fullest set), exact in the case that matters (a set near its limit).
uint64_t ElemTable::tight_id_bound(jg_ctx* ctx, DevBuf& cub_temp) {
    if (set_cap == 0) return id_bound = 0;
    ensure(idmax, 16);
    const uint32_t* nx = next_id.as<uint32_t>();
    const int n_sets = cub_count(set_cap, "sets");
    cub_run(cub_in(cub_temp), [&](void* temp, size_t& bytes) {
        return hipcub::DeviceReduce::Max(temp, bytes, nx, idmax.as<uint32_t>(), n_sets, ctx->stream);
    });
    pin_get(ctx, 0, idmax.p, 4);
    pin_sync(ctx);
    uint32_t mx;
    std::memcpy(&mx, pin_at(ctx, 0), 4);
    return id_bound = mx;
}

void ElemTable::names_added(uint64_t n, uint64_t pool_used_now, uint64_t next_id_bound) {
    id_bound = std::max(id_bound, next_id_bound);
    n_names += n;
    pool_used = pool_used_now;
    if (!marks.empty() && marks.back().first == n_names) return;
    marks.emplace_back(n_names, pool_used);
    if (marks.size() > 4096) marks.erase(marks.begin(), marks.begin() + 2048);
}

void ElemTable::issue_names(jg_ctx* ctx, uint64_t n_new, uint64_t pool_used_now) {
    names_added(n_new, pool_used_now, id_bound + n_new);
    g1 = n_names;
    p1 = pool_used;
    queue_names(ctx, *this);
}

}  // namespace jg

extern "C" {

int jg_orset_resolve_names(jg_orset* s, uint64_t n, const uint32_t* set, const uint64_t* off, const uint8_t* bytes, const uint8_t* is_null,
                           uint32_t* elem) {
    return jg::guard([&] {
        auto lk_ = jg::lock(s);  // calls on one context are serialised (shared scratch, stream)
        JG_REQUIRE(s, JG_EINVAL, "jg_orset_resolve_names: store is NULL");
        if (n == 0) return;
        JG_REQUIRE(elem, JG_EINVAL, "jg_orset_resolve_names: NULL argument");
        JG_REQUIRE(n < 0x7FFFFFF0ull, JG_EINVAL, "jg_orset_resolve_names: at most 2^31 names per call");
        check_names("jg_orset_resolve_names", n, set, off, bytes, is_null);
        jg_ctx* ctx = s->ctx;
        jg::ensure_device(ctx);
        Packed P(n, 0, set, off, bytes);
        const Resolved r = resolve_on_device(s, P, n, is_null);
        JG_HIP(hipMemcpyAsync(elem, r.elem, n * 4, hipMemcpyDeviceToHost, ctx->stream));
        JG_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int jg_orset_contains_names(jg_orset* s, uint64_t n, const uint32_t* set, const uint64_t* off, const uint8_t* bytes, const uint8_t* is_null,
                            uint8_t* out) {
    return jg::guard([&] {
        auto lk_ = jg::lock(s);
        JG_REQUIRE(s, JG_EINVAL, "jg_orset_contains_names: store is NULL");
        if (n == 0) return;
        JG_REQUIRE(out, JG_EINVAL, "jg_orset_contains_names: NULL argument");
        JG_REQUIRE(n < 0x7FFFFFF0ull, JG_EINVAL, "jg_orset_contains_names: at most 2^31 names per call");
        check_names("jg_orset_contains_names", n, set, off, bytes, is_null);
        jg_ctx* ctx = s->ctx;
        jg::ensure_device(ctx);
        jg::sync_counts(s);
        Packed P(n, 0, set, off, bytes);
        const Resolved r = resolve_on_device(s, P, n, is_null);
        jg::orset_contains_device(s, r.q, n, r.out);  // the query keys never leave the device
        JG_HIP(hipMemcpyAsync(out, r.out, n, hipMemcpyDeviceToHost, ctx->stream));
        JG_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int jg_orset_lookup_all_names(jg_orset* s, uint64_t n, const uint32_t* set, uint64_t* off, uint64_t* n_bytes, uint64_t* name_off, uint8_t* bytes,
                              uint8_t* is_null, uint32_t* elems, uint64_t cap_elems, uint64_t cap_bytes) {
    return jg::guard([&] {
        auto lk_ = jg::lock(s);
        JG_REQUIRE(s && off && n_bytes, JG_EINVAL, "jg_orset_lookup_all_names: NULL argument");
        off[0] = 0;
        *n_bytes = 0;
        if (n == 0) return;
        JG_REQUIRE(set, JG_EINVAL, "jg_orset_lookup_all_names: NULL set list");
        JG_REQUIRE(n < 0x7FFFFFF0ull, JG_EINVAL, "jg_orset_lookup_all_names: at most 2^31 sets per call");
        const bool query = !name_off && !bytes && !is_null;
        JG_REQUIRE(query || (name_off && is_null), JG_EINVAL, "jg_orset_lookup_all_names: name_off, bytes and is_null go together");
        jg_ctx* ctx = s->ctx;
        jg::ensure_device(ctx);
        jg::sync_counts(s);
        jg::ElemTable& T = *jg::orset_elem_table(s, true);
        T.ensure_names(ctx, 0, 0);
        // the members: jg_orset_lookup_all's count pass, offsets by a device scan, its write pass
        auto* st = static_cast<uint8_t*>(jg::scratch(ctx, ctx->scratch, (n + 1) * 8 + n * 4 + 64));
        auto* dmoff = reinterpret_cast<unsigned long long*>(st);
        auto* dset = reinterpret_cast<uint32_t*>(st + (n + 1) * 8);
        JG_HIP(hipMemcpyAsync(dset, set, n * 4, hipMemcpyHostToDevice, ctx->stream));
        JG_HIP(hipMemsetAsync(dmoff + n, 0, 8, ctx->stream));
        jg::orset_lookup_all_device(s, dset, n, reinterpret_cast<uint64_t*>(dmoff), nullptr);
        scan_in_place(ctx, dmoff, n + 1);
        JG_HIP(hipMemcpyAsync(off, dmoff, (n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
        JG_HIP(hipStreamSynchronize(ctx->stream));
        const uint64_t total = off[n];
        if (total == 0) return;
        JG_REQUIRE(total < 0x7FFFFFF0ull, JG_ESTATE, "jg_orset_lookup_all_names: more than 2^31 members in one call");
        // their names: lengths through the (set, id) index, offsets by a scan
        unsigned long long* dnoff;
        uint32_t *delem, *dg;
        uint8_t* dnull;
        jg::Layout L;
        L.add(dnoff, total + 2, 8), L.add(delem, total, 4), L.add(dg, total, 4), L.add(dnull, total, 1);
        L.bind(jg::scratch(ctx, ctx->scratch2, L.bytes() + 64));
        auto* dmiss = dnoff + total + 1;  // raised by a member whose id has no name
        JG_HIP(hipMemsetAsync(dnoff + total, 0, 16, ctx->stream));
        jg::orset_lookup_all_device(s, dset, n, reinterpret_cast<uint64_t*>(dmoff), delem);
        hipLaunchKernelGGL(k_nm_lens, dim3(blocks_for(total)), dim3(kBlock), 0, ctx->stream, T.view(), reinterpret_cast<const uint64_t*>(dmoff), n, dset,
                           delem, total, dg, dnoff, dnull, dmiss);
        JG_HIP(hipGetLastError());
        scan_in_place(ctx, dnoff, total + 1);
        jg::pin_get(ctx, 0, dnoff + total, 8);
        jg::pin_get(ctx, 8, dmiss, 8);
        jg::pin_sync(ctx);
        const uint64_t nb = *static_cast<const uint64_t*>(jg::pin_at(ctx, 0));
        const bool missing = *static_cast<const uint64_t*>(jg::pin_at(ctx, 8)) != 0;
        *n_bytes = nb;
        JG_REQUIRE(!missing, JG_ESTATE, "jg_orset_lookup_all_names: a member's id has no name in the element table");
        if (query) return;
        JG_REQUIRE(total <= cap_elems && nb <= cap_bytes && (bytes || nb == 0), JG_ESTATE,
                   "jg_orset_lookup_all_names: %llu members / %llu bytes exceed the buffers (%llu, %llu)", (unsigned long long)total,
                   (unsigned long long)nb, (unsigned long long)cap_elems, (unsigned long long)cap_bytes);
        if (nb) {
            auto* dbytes = static_cast<uint8_t*>(jg::scratch(ctx, ctx->scratch3, nb + 64));
            hipLaunchKernelGGL(k_nm_copy, dim3(blocks_for(nb)), dim3(kBlock), 0, ctx->stream, T.view(), dnoff, dg, total, nb, dbytes);
            JG_HIP(hipGetLastError());
            JG_HIP(hipMemcpyAsync(bytes, dbytes, nb, hipMemcpyDeviceToHost, ctx->stream));
        }
        JG_HIP(hipMemcpyAsync(name_off, dnoff, (total + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
        JG_HIP(hipMemcpyAsync(is_null, dnull, total, hipMemcpyDeviceToHost, ctx->stream));
        if (elems) JG_HIP(hipMemcpyAsync(elems, delem, total * 4, hipMemcpyDeviceToHost, ctx->stream));
        JG_HIP(hipStreamSynchronize(ctx->stream));
    });
}

}  // extern "C"

// jg_orset_apply_ops_names under the context lock, for it and for update.hip (the OR-Set commands of a batch by key).
void jg::orset_apply_ops_names_locked(jg_orset* s, uint64_t n_ops, const uint32_t* set, const uint8_t* op, const uint64_t* off, const uint8_t* bytes,
                                      const uint8_t* is_null, const uint64_t* tag_lo, const uint64_t* tag_hi, uint8_t* result, uint32_t* elem_out,
                                      uint64_t* add_lim, uint64_t* rem_lim, bool reads) {
    jg::require_writable(s, "jg_orset_apply_ops_names");
    JG_REQUIRE(s, JG_EINVAL, "jg_orset_apply_ops_names: store is NULL");
    if (n_ops == 0) return;
    const uint64_t n = n_ops;
    JG_REQUIRE(op && tag_lo && tag_hi && result, JG_EINVAL, "jg_orset_apply_ops_names: NULL argument");
    JG_REQUIRE(!add_lim == !rem_lim, JG_EINVAL, "jg_orset_apply_ops_names: add_lim and rem_lim go together");
    JG_REQUIRE(n < 0x7FFFFFF0ull, JG_EINVAL, "jg_orset_apply_ops_names: at most 2^31 ops per call");
    const uint64_t n_sets = check_names("jg_orset_apply_ops_names", n, set, off, bytes, is_null);
    for (uint64_t i = 0; i < n; ++i)
        JG_REQUIRE(op[i] >= 1 && (op[i] <= 3 || (reads && op[i] == 4)), JG_EINVAL,
                   "jg_orset_apply_ops_names: op[%llu] = %u is not 1 (Add), 2 (Remove) or 3 (Clear)", (unsigned long long)i, op[i]);
    jg_ctx* ctx = s->ctx;
    jg::ensure_device(ctx);
    jg::sync_counts(s);

    // each op's Clear epoch (the Clears of its set before it) and the sets Cleared, with their counts
    std::vector<uint32_t> epoch(n), cset, ccnt;
    uint64_t n_add = 0;
    {
        const bool dense = n_sets < 4 * n + 65536;
        std::vector<uint32_t> cnt(dense ? n_sets : 0, 0u);
        std::unordered_map<uint32_t, uint32_t> sparse;
        for (uint64_t i = 0; i < n; ++i) {
            uint32_t& c = dense ? cnt[set[i]] : sparse[set[i]];
            epoch[i] = c;
            if (op[i] == 3 && c++ == 0) cset.push_back(set[i]);
            n_add += op[i] == 1 && !is_null[i];
        }
        for (uint32_t c : cset) ccnt.push_back(dense ? cnt[c] : sparse[c]);
    }
    const uint64_t nc = cset.size();
    Packed P(n, nc, set, off, bytes);
    std::memcpy(P.epoch(), epoch.data(), n * 4);
    if (nc) std::memcpy(P.cset(), cset.data(), nc * 4), std::memcpy(P.ccnt(), ccnt.data(), nc * 4);
    for (uint64_t i = 0; i < n; ++i) P.meta()[i] = (uint8_t)((is_null[i] ? 1 : 0) | op[i] << 1);

    // every allocation first: room for the sets, the tables, the call's own block
    jg::ElemTable& T = *jg::orset_elem_table(s, true);
    T.ensure_sets(ctx, n_sets);
    T.ensure_names(ctx, 0, 0);
    JG_REQUIRE(!jg::orset_wave_open(s), JG_EINVAL, "jg_orset_apply_ops_names: a wave is open");
    const uint64_t ccap = jg::pow2_at_least(2 * n_add, 64);
    // the winners' sort orders on the set's bits and the op index (an unset key, all ones, sorts last either way)
    int key_bits = 32;
    while (key_bits < 64 && (n_sets - 1) >> (key_bits - 32)) ++key_bits;
    using ull = unsigned long long;
    const int n_i = jg::cub_count(n, "ops"), n1_i = jg::cub_count(n + 1, "ops");
    // the two scans and the sort share one workspace, one after the other on the stream
    const size_t tb = std::max(jg::cub_temp_bytes([&](void* temp, size_t& bytes) {
                                   return hipcub::DeviceRadixSort::SortKeys(temp, bytes, (const ull*)nullptr, (ull*)nullptr, n_i, 0, key_bits, ctx->stream);
                               }),
                               jg::cub_temp_bytes([&](void* temp, size_t& bytes) {
                                   return hipcub::DeviceScan::ExclusiveSum(temp, bytes, (ull*)nullptr, (ull*)nullptr, n1_i, ctx->stream);
                               }));
    uint8_t *dstage, *dtmp;
    Cand C{nullptr, nullptr, ccap - 1};
    ull *nkey, *cnt, *len, *wkey, *skey, *st;
    uint32_t *rid, *slot, *newid, *delem;
    jg::Layout L;
    L.add(dstage, P.h.size(), 8), L.add(C.slot, ccap, 8), L.add(nkey, n, 8), L.add(cnt, n + 1, 8), L.add(len, n + 1, 8), L.add(wkey, n, 8);
    L.add(skey, n, 8), L.add(st, 2, 8), L.add(C.first, ccap, 8), L.add(rid, n, 8), L.add(slot, n, 8), L.add(newid, n, 8), L.add(delem, n, 8);
    L.add(dtmp, tb + 64);
    jg::DevBuf blk;  // the call's own block: the record side below reuses the context's scratch
    blk.alloc(L.bytes());
    L.bind(blk.p);
    const Staged S = P.on(dstage);
    const auto* dcset = reinterpret_cast<const uint32_t*>(dstage + P.at_cset);
    const auto* dccnt = reinterpret_cast<const uint32_t*>(dstage + P.at_ccnt);

    // JANUS_TRACE_APPLY (as jg_orset_apply_ops): the launches' device time beside the record side's host line
    static const bool tr = std::getenv("JANUS_TRACE_APPLY") != nullptr;
    hipEvent_t ev[5] = {};
    auto stamp = [&](int k) {
        if (!tr) return;
        JG_HIP(hipEventCreate(&ev[k]));
        JG_HIP(hipEventRecord(ev[k], ctx->stream));
    };

    // resolve and intern (the table itself is only read)
    stamp(0);
    JG_HIP(hipMemcpyAsync(dstage, P.h.data(), P.h.size(), hipMemcpyHostToDevice, ctx->stream));
    stamp(1);
    JG_HIP(hipMemsetAsync(C.slot, 0, ccap * 8, ctx->stream));
    JG_HIP(hipMemsetAsync(C.first, 0xFF, ccap * 4, ctx->stream));
    JG_HIP(hipMemsetAsync(st, 0, 16, ctx->stream));
    const dim3 grid(blocks_for(n + 1)), block(kBlock);
    hipLaunchKernelGGL(k_nm_claim, grid, block, 0, ctx->stream, T.view(), T.kmask, T.salt, S, n, C, rid, nkey, slot);
    hipLaunchKernelGGL(k_nm_win, grid, block, 0, ctx->stream, S, n, C, slot, cnt, len, wkey);
    JG_HIP(hipGetLastError());
    const auto tmp = jg::cub_in(dtmp, tb);
    jg::cub_run(tmp, [&](void* temp, size_t& bytes) { return hipcub::DeviceScan::ExclusiveSum(temp, bytes, cnt, cnt, n1_i, ctx->stream); });
    jg::cub_run(tmp, [&](void* temp, size_t& bytes) { return hipcub::DeviceScan::ExclusiveSum(temp, bytes, len, len, n1_i, ctx->stream); });
    jg::cub_run(tmp, [&](void* temp, size_t& bytes) {
        return hipcub::DeviceRadixSort::SortKeys(temp, bytes, wkey, skey, n_i, 0, key_bits, ctx->stream);
    });
    hipLaunchKernelGGL(k_nm_assign, grid, block, 0, ctx->stream, T.view(), skey, n, newid, st);
    hipLaunchKernelGGL(k_nm_ids, grid, block, 0, ctx->stream, S, n, C, rid, nkey, slot, newid, delem);
    JG_HIP(hipGetLastError());
    stamp(2);
    std::vector<uint32_t> elem(n);
    JG_HIP(hipMemcpyAsync(elem.data(), delem, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    jg::pin_get(ctx, 0, cnt + n, 8);
    jg::pin_get(ctx, 8, len + n, 8);
    jg::pin_get(ctx, 16, st, 16);
    jg::pin_sync(ctx);
    const auto* hw = static_cast<const uint64_t*>(jg::pin_at(ctx, 0));
    const uint64_t n_new = hw[0], new_bytes = hw[1], over = hw[2], id_bound = hw[3];
    JG_REQUIRE(!over, JG_ESTATE, "jg_orset_apply_ops_names: a set has no element ids left");
    if (n_new) T.ensure_names(ctx, n_new, new_bytes);  // growing rebuilds, it changes no content

    // the record side over the ids: jg_orset_apply_ops' walk and union; the table is unchanged if it refuses
    jg::orset_apply_ops_ids(s, n, set, elem.data(), op, tag_lo, tag_hi, result, add_lim, rem_lim);
    if (elem_out) std::memcpy(elem_out, elem.data(), n * 4);

    // the table: what jg_orset_names_sync would have been told
    stamp(3);
    if (n_new || nc) {
        if (n_new) hipLaunchKernelGGL(k_nm_put, grid, block, 0, ctx->stream, T.view(), T.n_names, T.pool_used, S, n, cnt, len, nkey, newid);
        hipLaunchKernelGGL(k_nm_sets, dim3(blocks_for(std::max(n, nc))), block, 0, ctx->stream, T.view(), skey, n, dcset, dccnt, nc);
        JG_HIP(hipGetLastError());
        stamp(4);
        JG_HIP(hipStreamSynchronize(ctx->stream));
        T.names_added(n_new, T.pool_used + new_bytes, id_bound);
    }
    if (tr) {
        float up = 0, res = 0, put = 0;
        JG_HIP(hipEventElapsedTime(&up, ev[0], ev[1]));
        JG_HIP(hipEventElapsedTime(&res, ev[1], ev[2]));
        if (ev[4]) JG_HIP(hipEventElapsedTime(&put, ev[3], ev[4]));
        std::fprintf(stderr, "orset apply_ops_names(%llu ops, %llu name bytes, %llu new names): upload %.3f ms, resolve + intern launches %.3f ms, "
                     "put launches %.3f ms\n", (unsigned long long)n, (unsigned long long)off[n], (unsigned long long)n_new, up, res, put);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
}

extern "C" {

int jg_orset_apply_ops_names(jg_orset* s, uint64_t n_ops, const uint32_t* set, const uint8_t* op, const uint64_t* off, const uint8_t* bytes,
                             const uint8_t* is_null, const uint64_t* tag_lo, const uint64_t* tag_hi, uint8_t* result, uint32_t* elem_out,
                             uint64_t* add_lim, uint64_t* rem_lim) {
    return jg::guard([&] {
        auto lk_ = jg::lock(s);
        jg::orset_apply_ops_names_locked(s, n_ops, set, op, off, bytes, is_null, tag_lo, tag_hi, result, elem_out, add_lim, rem_lim, false);
    });
}

int jg_orset_names_sync(jg_orset* s, uint64_t n_sets, const uint32_t* set, const uint32_t* next_id, const uint8_t* cleared, uint64_t n_names,
                        const uint32_t* name_set, const uint32_t* name_id, const uint64_t* off, const uint8_t* bytes) {
    return jg::guard([&] {
        auto lk_ = jg::lock(s);  // calls on one context are serialised (shared scratch, stream)
        jg::require_writable(s, "jg_orset_names_sync");
        JG_REQUIRE(s, JG_EINVAL, "jg_orset_names_sync: store is NULL");
        JG_REQUIRE((n_sets == 0 || (set && next_id && cleared)) && (n_names == 0 || (name_set && name_id && off && bytes)), JG_EINVAL,
                   "jg_orset_names_sync: NULL argument");
        JG_REQUIRE(n_names == 0 || off[0] == 0, JG_EINVAL, "jg_orset_names_sync: off[0] must be 0");
        jg_ctx* ctx = s->ctx;
        jg::ensure_device(ctx);
        jg::ElemTable& T = *jg::orset_elem_table(s, true);
        JG_REQUIRE(!jg::orset_wave_open(s), JG_EINVAL, "jg_orset_names_sync: a wave is open");
        uint64_t mx = 0, idb = 0;
        for (uint64_t i = 0; i < n_sets; ++i) mx = std::max<uint64_t>(mx, (uint64_t)set[i] + 1), idb = std::max<uint64_t>(idb, next_id[i]);
        for (uint64_t i = 0; i < n_names; ++i) {
            JG_REQUIRE(off[i + 1] >= off[i] && off[i + 1] - off[i] < 0x7FFFFFFFull, JG_EINVAL, "jg_orset_names_sync: bad offsets at name %llu",
                       (unsigned long long)i);
            JG_REQUIRE(name_id[i] < JG_NULL_ELEM - 1, JG_EINVAL, "jg_orset_names_sync: id %u out of range", name_id[i]);
            mx = std::max<uint64_t>(mx, (uint64_t)name_set[i] + 1);
        }
        if (mx == 0) return;
        T.ensure_sets(ctx, mx);
        const uint64_t nb = n_names ? off[n_names] : 0;
        T.ensure_names(ctx, n_names, nb);
        uint32_t *d_set, *d_next, *d_nset, *d_nid;
        uint64_t* d_off;
        uint8_t* d_clr;
        jg::Layout L;
        L.add(d_set, n_sets, 4), L.add(d_next, n_sets, 4), L.add(d_nset, n_names, 4), L.add(d_nid, n_names, 4);
        L.add(d_off, n_names + 1, 16), L.add(d_clr, n_sets, 1);
        L.bind(jg::scratch(ctx, ctx->scratch, L.bytes() + 64));
        if (n_sets) {
            JG_HIP(hipMemcpyAsync(d_set, set, n_sets * 4, hipMemcpyHostToDevice, ctx->stream));
            JG_HIP(hipMemcpyAsync(d_next, next_id, n_sets * 4, hipMemcpyHostToDevice, ctx->stream));
            JG_HIP(hipMemcpyAsync(d_clr, cleared, n_sets, hipMemcpyHostToDevice, ctx->stream));
            hipLaunchKernelGGL(k_sets_update, dim3(blocks_for(n_sets)), dim3(kBlock), 0, ctx->stream, T.view(), d_set, d_next, d_clr, n_sets);
            JG_HIP(hipGetLastError());
        }
        if (n_names) {
            JG_HIP(hipMemcpyAsync(d_nset, name_set, n_names * 4, hipMemcpyHostToDevice, ctx->stream));
            JG_HIP(hipMemcpyAsync(d_nid, name_id, n_names * 4, hipMemcpyHostToDevice, ctx->stream));
            JG_HIP(hipMemcpyAsync(d_off, off, (n_names + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
            if (nb) JG_HIP(hipMemcpyAsync(T.pool.as<uint8_t>() + T.pool_used, bytes, nb, hipMemcpyHostToDevice, ctx->stream));
            hipLaunchKernelGGL(k_names_put, dim3(blocks_for(n_names)), dim3(kBlock), 0, ctx->stream, T.view(), T.n_names, T.pool_used, d_nset, d_nid,
                               d_off, n_names, T.kmask, T.salt);
            JG_HIP(hipGetLastError());
        }
        JG_HIP(hipStreamSynchronize(ctx->stream));
        T.names_added(n_names, T.pool_used + nb, idb);
    });
}

int jg_orset_wave_names(jg_orset* s, uint64_t* n_names, uint64_t* n_bytes, uint32_t* set, uint32_t* id, uint64_t* off, uint8_t* bytes) {
    return jg::guard([&] {
        auto lk_ = jg::lock(s);  // calls on one context are serialised (shared scratch, stream)
        JG_REQUIRE(s && n_names && n_bytes, JG_EINVAL, "jg_orset_wave_names: NULL argument");
        jg::ElemTable* T = jg::orset_elem_table(s, false);
        const uint64_t n = T ? T->g1 - T->g0 : 0, nb = T ? T->p1 - T->p0 : 0;
        *n_names = n;
        *n_bytes = nb;
        if (!set || n == 0) return;
        JG_REQUIRE(id && off && (bytes || nb == 0), JG_EINVAL, "jg_orset_wave_names: NULL buffer");
        jg_ctx* ctx = s->ctx;
        jg::ensure_device(ctx);
        const auto& o = T->nout;
        // queued by the commit: wait for that copy; or the staging was reused since (a names_since pull): staged again
        if (o.g0 != o.g1 && o.g0 == T->g0 && o.g1 == T->g1 && o.p0 == T->p0 && o.p1 == T->p1) JG_HIP(hipEventSynchronize(o.ev));
        else names_stage_now(ctx, *T, T->g0, T->g1, T->p0, T->p1, "jg_orset_wave_names");
        jg::NamesStaging(n, nb).copy_out(o.host, T->p0, set, id, off, bytes);
    });
}

int jg_orset_names_since(jg_orset* s, uint64_t from, uint64_t* to, uint64_t* n_bytes, uint32_t* set, uint32_t* id, uint64_t* off, uint8_t* bytes) {
    return jg::guard([&] {
        auto lk_ = jg::lock(s);
        JG_REQUIRE(s && to && n_bytes, JG_EINVAL, "jg_orset_names_since: NULL argument");
        jg::ElemTable* T = jg::orset_elem_table(s, false);
        const uint64_t total = T ? T->n_names : 0;
        JG_REQUIRE(from <= total, JG_EINVAL, "jg_orset_names_since: from %llu past the %llu names held", (unsigned long long)from,
                   (unsigned long long)total);
        *to = total;
        *n_bytes = 0;
        const uint64_t n = total - from;
        if (n == 0) return;
        jg_ctx* ctx = s->ctx;
        jg::ensure_device(ctx);
        // A commit's new names take their pool bytes by atomics (not in name order), so the bytes of names
        // [from, total) lie in the pool range that starts at the last mark at or before `from` (every name
        // past a mark was made after it) and ends at pool_used.  One queue of copies into page-locked
        // staging, one wait; kept for the second call of a size query + fill.
        uint64_t pool0 = 0;
        for (auto it = T->marks.rbegin(); it != T->marks.rend(); ++it)
            if (it->first <= from) { pool0 = it->second; break; }
        names_stage_now(ctx, *T, from, total, pool0, T->pool_used, "jg_orset_names_since");
        const auto& o = T->nout;
        *n_bytes = o.since_bytes;
        if (!set) return;
        JG_REQUIRE(id && off && (bytes || o.since_bytes == 0), JG_EINVAL, "jg_orset_names_since: NULL buffer");
        jg::NamesStaging(n, o.since_pool1 - o.since_pool0).copy_out(o.host, o.since_pool0, set, id, off, bytes);
    });
}

}  // extern "C"
