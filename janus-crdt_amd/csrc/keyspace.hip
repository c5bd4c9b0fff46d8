// keyspace.hip — jg_keyspace: KeySpaceManager's state (BFT-CRDT/CRDTManagers/KeySpaceManager.cs): the set, the
// keySpaces dictionary and the LastKeySpaceSet watermark.  Every entry is key + "\0" + guid in the set's pool, so a
// dictionary entry holds no bytes of its own: (string id of the entry that introduced the key, key length, guid).
// Nothing leaves either HashSet, so "LookupAll().Except(LastKeySpaceSet)" (:157-159) is the present entries from the add
// ordinal the last OnNext ended at.
//
// Owns the dictionary, the journal and the watermark; the set is tpset.hip's and is written through its bodies
// (tpset_host.hpp) only.  A batch of items (OnNext's new entries, or CreateNewKVPair's keys) goes
//   k_ks_parse | k_ks_local -> k_ks_find -> k_ks_win -> two count scans -> (totals read back) -> k_ks_commit
#include <memory>
#include <vector>

#include "tpset_host.hpp"
#include "wire_cursor.hpp"

using namespace jgt;

namespace {

using jg::blocks_for;

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

// item o's key equals the key k of klen bytes hashed to `key` (the call-wide table's equality, tpset_dict.hpp)
struct SameKey {
    const Store& S;
    const Items& I;
    ull key;
    const uint8_t* k;
    uint32_t klen;
    __device__ bool operator()(uint32_t o) const { return I.key[o] == key && I.klen[o] == klen && same_bytes(S.pool + S.soff[I.sid[o]], k, klen); }
};

// first wins: among the well-formed items whose key the dictionary lacks, the smallest index per distinct key
__global__ void k_ks_find(Store S, Dict D, Items I) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= I.n || !I.valid[i] || I.status[i]) return;
    const uint8_t* k = S.pool + S.soff[I.sid[i]];
    const uint32_t klen = I.klen[i];
    if (dict_find(S, D, I.key[i], k, klen) != kNone) return;
    const uint32_t slot = claim_slot(I.prep, I.pmask, I.key[i], (uint32_t)i, SameKey{S, I, I.key[i], k, klen});
    atomicMin(&I.pmin[slot], (uint32_t)i);
    I.slot[i] = slot;
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
        if (j) {
            const uint32_t slot = find_slot(I.prep, I.pmask, I.key[i], SameKey{S, I, I.key[i], k, klen});
            if (slot != kNone) j = I.pmin[slot] > i;
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
    const uint64_t slots = jg::pow2_at_least(2 * n, 64);
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
    jg_ctx* ctx = ks->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t n = B.I.n, slots = B.I.pmask + 1;
    const unsigned g = blocks_for(n);
    JG_HIP(hipMemsetAsync(B.I.prep, 0, slots * 4, st));
    JG_HIP(hipMemsetAsync(B.I.pmin, 0xFF, slots * 4, st));
    hipLaunchKernelGGL(k_ks_find, dim3(g), dim3(kBlock), 0, st, s->view(), ks->dict(), B.I);
    hipLaunchKernelGGL(k_ks_win, dim3(g), dim3(kBlock), 0, st, s->view(), ks->dict(), B.I, B.added, B.jrn);
    excl_scan(ctx, s->wscan, B.added, B.oa, n);
    excl_scan(ctx, s->wscan, B.jrn, B.oj, n);
    JG_HIP(hipGetLastError());
    const auto [ta, tj] = read_totals(ctx, B.oa + n, B.oj + n);
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
    cv.bind(work(ks->ctx, ks->wk, cv.bytes() + 1024));
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
        auto lk_ = jg::lock(ctx);
        std::unique_ptr<jg_keyspace> ks(new jg_keyspace());
        std::unique_ptr<jg_tpset> set(tpset_create(ctx, cap_keys, cap_bytes));  // freed with ks if an allocation below throws
        ks->ctx = ctx;
        ks->cap = cap_keys;
        const uint64_t slots = jg::pow2_at_least(2 * (cap_keys + 2), 64);
        ks->mask = slots - 1;
        const uint64_t n = cap_keys + 2;
        ks->table.alloc(slots * 4), ks->dsid.alloc(n * 4), ks->dklen.alloc(n * 4), ks->dglo.alloc(n * 8), ks->dghi.alloc(n * 8), ks->dkey.alloc(n * 8);
        ks->jsid.alloc(n * 4), ks->jlen.alloc(n * 4), ks->jglo.alloc(n * 8), ks->jghi.alloc(n * 8), ks->jstatus.alloc(n);
        JG_HIP(hipMemsetAsync(ks->table.p, 0, slots * 4, ctx->stream));
        JG_HIP(hipStreamSynchronize(ctx->stream));
        ks->set = set.release();
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
        tpset_apply_ops(ks->set, n, op.data(), eoff.data(), ent.data(), nullptr, nullptr);
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
        cv.bind(work(ks->ctx, ks->wk, cv.bytes() + 1024));
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
            try {
                tpset_merge_json(ks->set, 1, o, bytes + off[m], mode, &bad, &part);
            } catch (const jg::Error& e) {  // the reference's Decode / Merge throws before OnNext: the watermark stays
                if (bad_msg && e.code == JG_EINVAL) *bad_msg = m;
                if (partial) *partial = part;
                if (n_new) *n_new = total;
                jg::fail(e.code, "jg_keyspace_receive: message %llu: %s", (ull)m, e.msg.c_str());
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
        jg_ctx* ctx = ks->ctx;
        hipStream_t st = ctx->stream;
        jg::ensure_device(ctx);
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
        cv.bind(work(ctx, ks->wk, cv.bytes() + 1024));
        excl_scan(ctx, s->wscan, ks->jlen.as<uint32_t>() + from, ob, n);
        if (!query)
            hipLaunchKernelGGL(k_ks_journal, dim3(blocks_for(n)), dim3(kBlock), 0, st, s->view(), from, n, ks->jsid.as<uint32_t>(), ks->jlen.as<uint32_t>(),
                               ks->jglo.as<ull>(), ks->jghi.as<ull>(), ks->jstatus.as<uint8_t>(), ob, d_off, d_bytes, d_guid, d_status);
        JG_HIP(hipGetLastError());
        const uint64_t nb = read_totals(ctx, ob + n)[0];
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
        cv.bind(work(ks->ctx, ks->wk, cv.bytes() + 1024));
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
