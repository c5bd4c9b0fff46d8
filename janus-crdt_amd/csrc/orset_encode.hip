// orset_encode.hip — ORSetMsg.Encode on the device (jg_orset_encode_json; ORSet.cs:56-69, 305-308).  It shares the
// store's element table (orset_names.hpp) and three buffers of jg_orset_wire (orset_wave.hpp) with the wave path,
// nothing else.
//
// {"addSet":{"<e>":[<tags>],...},"removeSet":{...},"nullAddGuid":[<tags>],"nullRemoveGuid":[<tags>]} in
// System.Text.Json's compact form: addSet elements in ascending element id (the add Dictionary's insertion
// order), removeSet elements by their first tombstone's ord (when the element entered the remove Dictionary),
// ties by id, tags by (ord, tag) (HashSet<Guid> insertion order), the null element's tags in the two lists.
// Runs = the kept records of one (query, side, element); sections: 0 addSet, 1 removeSet, 2 nullAddGuid,
// 3 nullRemoveGuid; seg = query * 4 + section.
#include <hipcub/hipcub.hpp>

#include "orset_wave.hpp"

namespace {

constexpr uint32_t kEncFixed = 65;                           // the five fixed texts of one ORSetMsg
__constant__ const uint32_t kEncBefore[4] = {11, 26, 43, 63};  // fixed bytes before each section

// JavaScriptEncoder.Default for a UTF-8 element string (host/wire.cpp escape): its escaped length, or its bytes.
template <bool WRITE>
__device__ uint32_t enc_escape(const uint8_t* s, uint32_t len, uint8_t* o) {
    const char* HX = "0123456789ABCDEF";
    uint32_t n = 0;
    auto unit = [&](uint32_t u) {
        if (WRITE) {
            o[n] = '\\', o[n + 1] = 'u', o[n + 2] = HX[u >> 12 & 15], o[n + 3] = HX[u >> 8 & 15], o[n + 4] = HX[u >> 4 & 15], o[n + 5] = HX[u & 15];
        }
        n += 6;
    };
    for (uint32_t i = 0; i < len;) {
        const uint32_t c = s[i];
        if (c >= 0x80) {
            const uint32_t k = c >= 0xF0 ? 4 : c >= 0xE0 ? 3 : 2;
            uint32_t cp = c & (k == 4 ? 0x07 : k == 3 ? 0x0F : 0x1F);
            for (uint32_t q = 1; q < k && i + q < len; ++q) cp = cp << 6 | (s[i + q] & 0x3F);
            i += k;
            if (cp >= 0x10000) {
                unit(0xD800 | (cp - 0x10000) >> 10);
                unit(0xDC00 | ((cp - 0x10000) & 0x3FF));
            } else {
                unit(cp);
            }
            continue;
        }
        ++i;
        char e = 0;
        if (c == '\\') e = '\\';
        else if (c == '\b') e = 'b';
        else if (c == '\t') e = 't';
        else if (c == '\n') e = 'n';
        else if (c == '\f') e = 'f';
        else if (c == '\r') e = 'r';
        if (e) {
            if (WRITE) o[n] = '\\', o[n + 1] = e;
            n += 2;
        } else if (c < 0x20 || c == 0x7F || c == '"' || c == '&' || c == '\'' || c == '+' || c == '<' || c == '>' || c == '`') {
            unit(c);
        } else {
            if (WRITE) o[n] = (uint8_t)c;
            ++n;
        }
    }
    return n;
}

__device__ __forceinline__ void enc_put(uint8_t* o, const char* s) {
    while (*s) *o++ = (uint8_t)*s++;
}

// "<Guid D>" (38 bytes): b3 b2 b1 b0 - b5 b4 - b7 b6 - b8 b9 - b10..b15, lower-case hex
__device__ __forceinline__ void enc_guid(uint8_t* o, unsigned long long lo, unsigned long long hi) {
    const char* hx = "0123456789abcdef";
    const int order[16] = {3, 2, 1, 0, 5, 4, 7, 6, 8, 9, 10, 11, 12, 13, 14, 15};
    int p = 0;
    o[p++] = '"';
    for (int k = 0; k < 16; ++k) {
        if (k == 4 || k == 6 || k == 8 || k == 10) o[p++] = '-';
        const uint32_t b = (uint32_t)((order[k] < 8 ? lo >> (8 * order[k]) : hi >> (8 * (order[k] - 8))) & 0xFF);
        o[p++] = hx[b >> 4];
        o[p++] = hx[b & 15];
    }
    o[p] = '"';
}

struct EncRec {  // the gathered records (jg::orset_gather_sets)
    const unsigned long long *key, *tlo, *thi;
    const uint32_t *ord, *qs;
};

// run heads over the kept records kidx[0..K) (K on the device); positions >= K are padding
__global__ void k_enc_heads(EncRec G, const uint32_t* __restrict__ kidx, const unsigned long long* __restrict__ K, uint64_t R, uint32_t* __restrict__ hf) {
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= R) return;
    uint32_t h = 0;
    if (j < *K) {
        const uint32_t r = kidx[j];
        h = j == 0 || G.key[kidx[j - 1]] != G.key[r] || G.qs[kidx[j - 1]] != G.qs[r];
    }
    hf[j] = h;
}

// per run (rid[j] - 1 = the run of kept record j): its first kept record, end, query / side / key; first ord reset
__global__ void k_enc_runs(EncRec G, const uint32_t* __restrict__ kidx, const unsigned long long* __restrict__ K, const uint32_t* __restrict__ rid,
                           uint32_t* __restrict__ rstart, uint32_t* __restrict__ rend, uint32_t* __restrict__ rfirst, unsigned long long* __restrict__ nruns) {
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t k = *K;
    if (j >= k) return;
    const uint32_t run = rid[j] - 1;
    if (j == 0 || rid[j - 1] != rid[j]) {
        rstart[run] = (uint32_t)j;
        rfirst[run] = 0xFFFFFFFFu;
        if (j > 0) rend[run - 1] = (uint32_t)j;
    }
    if (j + 1 == k) {
        rend[run] = (uint32_t)k;
        *nruns = run + 1;
    }
}

__global__ void k_enc_first_ord(EncRec G, const uint32_t* __restrict__ kidx, const unsigned long long* __restrict__ K, const uint32_t* __restrict__ rid,
                                uint32_t* __restrict__ rfirst) {
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= *K) return;
    const uint32_t o = G.ord[kidx[j]], run = rid[j] - 1;
    if (rfirst[run] > o) atomicMin(rfirst + run, o);
}

__device__ __forceinline__ uint32_t enc_section(uint32_t qs, unsigned long long key) {
    return ((uint32_t)key == JG_NULL_ELEM ? 2u : 0u) + (qs & 1u);
}

// run sort keys: seg << 32 | (removeSet ? first ord : 0), stable over runs in (query, side, id) order; padding ~0
__global__ void k_enc_run_keys(EncRec G, const uint32_t* __restrict__ kidx, const uint32_t* __restrict__ rstart, const uint32_t* __restrict__ rfirst,
                               const unsigned long long* __restrict__ nruns, uint64_t R, unsigned long long* __restrict__ rkey, uint32_t* __restrict__ rval) {
    const uint64_t run = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (run >= R) return;
    unsigned long long k = ~0ull;
    if (run < *nruns) {
        const uint32_t r = kidx[rstart[run]];
        const uint32_t qs = G.qs[r], sec = enc_section(qs, G.key[r]);
        const unsigned long long seg = (unsigned long long)(qs >> 1) * 4 + sec;
        k = seg << 32 | (sec == 1 ? rfirst[run] : 0u);
    }
    rkey[run] = k;
    rval[run] = (uint32_t)run;
}

// per run in output order (rank): its rank, record count, text length; the per-(query, section) bytes and first rank
__global__ void k_enc_run_len(EncRec G, Names N, const uint32_t* __restrict__ kidx, const uint32_t* __restrict__ rstart, const uint32_t* __restrict__ rend,
                              const unsigned long long* __restrict__ skey, const uint32_t* __restrict__ srun, const unsigned long long* __restrict__ nruns,
                              uint64_t R, uint32_t* __restrict__ rrank, unsigned long long* __restrict__ cnt, unsigned long long* __restrict__ tlen,
                              unsigned long long* __restrict__ qsec, uint32_t* __restrict__ sfirst, unsigned* __restrict__ err) {
    const uint64_t rank = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (rank >= R) return;
    if (rank >= *nruns) {
        cnt[rank] = 0;
        tlen[rank] = 0;
        return;
    }
    const uint32_t run = srun[rank];
    rrank[run] = (uint32_t)rank;
    const uint32_t c = rend[run] - rstart[run];
    const unsigned long long key = G.key[kidx[rstart[run]]];
    const uint32_t seg = (uint32_t)(skey[rank] >> 32), sec = seg & 3;
    unsigned long long len = 38ull * c + (c - 1);
    if (sec < 2) {
        const uint32_t g = itab_find(N, (uint32_t)(key >> 32), (uint32_t)key);
        if (g == kNoName) {
            atomicOr(err, 1u);
        } else {
            len += 1 + enc_escape<false>(N.pool + N.off[g], N.len[g], nullptr) + 3 + 1;
            if (rank > 0 && (uint32_t)(skey[rank - 1] >> 32) == seg) len += 1;  // ',' before a later element
        }
    }
    cnt[rank] = c;
    tlen[rank] = len;
    atomicAdd(qsec + seg, len);
    if (sfirst[seg] > rank) atomicMin(sfirst + seg, (uint32_t)rank);
}

// record sort keys: output rank of its run << 32 | ord (stable: the store's tag order breaks ord ties); padding ~0
__global__ void k_enc_rec_keys(EncRec G, const uint32_t* __restrict__ kidx, const unsigned long long* __restrict__ K, const uint32_t* __restrict__ rid,
                               const uint32_t* __restrict__ rrank, uint64_t R, unsigned long long* __restrict__ key, uint32_t* __restrict__ val) {
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= R) return;
    key[j] = j < *K ? (unsigned long long)rrank[rid[j] - 1] << 32 | G.ord[kidx[j]] : ~0ull;
    val[j] = (uint32_t)j;
}

__global__ void k_enc_qlen(const unsigned long long* __restrict__ qsec, uint64_t n, unsigned long long* __restrict__ qlen) {
    const uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q < n) qlen[q] = kEncFixed + qsec[4 * q] + qsec[4 * q + 1] + qsec[4 * q + 2] + qsec[4 * q + 3];
    if (q == n) qlen[q] = 0;
}

// where a section's text starts in query q's state
__device__ __forceinline__ unsigned long long enc_sec_at(const unsigned long long* qoff, const unsigned long long* qsec, uint32_t q, uint32_t sec) {
    unsigned long long p = qoff[q] + kEncBefore[sec];
    for (uint32_t s = 0; s < sec; ++s) p += qsec[4 * q + s];
    return p;
}

__global__ void k_enc_fixed(const unsigned long long* __restrict__ qoff, const unsigned long long* __restrict__ qsec, uint64_t n, uint8_t* __restrict__ out) {
    const uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= n) return;
    uint8_t* o = out + qoff[q];
    enc_put(o, "{\"addSet\":{");
    enc_put(out + enc_sec_at(qoff, qsec, (uint32_t)q, 1) - 15, "},\"removeSet\":{");
    enc_put(out + enc_sec_at(qoff, qsec, (uint32_t)q, 2) - 17, "},\"nullAddGuid\":[");
    enc_put(out + enc_sec_at(qoff, qsec, (uint32_t)q, 3) - 20, "],\"nullRemoveGuid\":[");
    enc_put(out + qoff[q + 1] - 2, "]}");
}

// each run's element header / closing bracket; rtags[rank] = where its first tag goes
__global__ void k_enc_run_text(EncRec G, Names N, const uint32_t* __restrict__ kidx, const uint32_t* __restrict__ rstart,
                               const unsigned long long* __restrict__ skey, const uint32_t* __restrict__ srun, const unsigned long long* __restrict__ nruns,
                               const unsigned long long* __restrict__ rpos, const unsigned long long* __restrict__ tlen, const uint32_t* __restrict__ sfirst,
                               const unsigned long long* __restrict__ qoff, const unsigned long long* __restrict__ qsec, unsigned long long* __restrict__ rtags,
                               uint8_t* __restrict__ out) {
    const uint64_t rank = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (rank >= *nruns) return;
    const uint32_t seg = (uint32_t)(skey[rank] >> 32), sec = seg & 3, q = seg >> 2;
    unsigned long long p = enc_sec_at(qoff, qsec, q, sec) + (rpos[rank] - rpos[sfirst[seg]]);
    if (sec < 2) {
        const unsigned long long key = G.key[kidx[rstart[srun[rank]]]];
        const uint32_t g = itab_find(N, (uint32_t)(key >> 32), (uint32_t)key);
        if (rank > 0 && (uint32_t)(skey[rank - 1] >> 32) == seg) out[p++] = ',';
        out[p++] = '"';
        p += enc_escape<true>(N.pool + N.off[g], N.len[g], out + p);
        out[p++] = '"', out[p++] = ':', out[p++] = '[';
        out[enc_sec_at(qoff, qsec, q, sec) + (rpos[rank] - rpos[sfirst[seg]]) + tlen[rank] - 1] = ']';
    }
    rtags[rank] = p;
}

// each record's tag text: ',' before every tag but a run's first
__global__ void k_enc_rec_text(EncRec G, const uint32_t* __restrict__ kidx, const unsigned long long* __restrict__ K, const uint32_t* __restrict__ srec,
                               const uint32_t* __restrict__ rid, const uint32_t* __restrict__ rrank, const unsigned long long* __restrict__ cpos,
                               const unsigned long long* __restrict__ rtags, uint8_t* __restrict__ out) {
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= *K) return;
    const uint32_t j = srec[p], rank = rrank[rid[j] - 1], r = kidx[j];
    const unsigned long long k = p - cpos[rank];
    unsigned long long at = rtags[rank] + 39 * k;
    if (k) out[at - 1] = ',';
    enc_guid(out + at, G.tlo[r], G.thi[r]);
}

// jg_orset_encode_json: gather the sets' records below the limits, order them (runs by section and element, tags
// by ord), size every state, then write them (see the header comment).  Two round trips: the record
// count (gather) and the states' offsets; a third copy brings the bytes.
//
// The size phase: everything up to the states' offsets (P.qoff, on the device) and the missing-name flag, which it
// queues into the page-locked bytes at 0; the caller's pin_sync brings it.  The plan (jg_orset_wire::enc_plan) is what
// the write phase needs of it: it holds until the next size phase on the store.
void encode_size(jg_orset* s, uint64_t n, const uint32_t* set, const uint64_t* add_lim, const uint64_t* rem_lim) {
    jg_ctx* ctx = s->ctx;
    jg::orset_elem_table(s, true)->ensure_names(ctx, 0, 0);  // a store that never saw a name: empty tables
    jg_orset_wire* w = s->wire;
    const Names N = w->names.view();
    const bool lim = add_lim != nullptr;
    using ull = unsigned long long;
    uint32_t* d_sets;
    ull* d_lim;
    jg::Layout Q;
    Q.add(d_sets, n), Q.add(d_lim, lim ? 2 * n : 0);
    Q.bind(jg::scratch(ctx, ctx->scratch, Q.bytes() + 256));
    if (!lim) d_lim = nullptr;
    JG_HIP(hipMemcpyAsync(d_sets, set, n * 4, hipMemcpyHostToDevice, ctx->stream));
    if (lim) {
        std::vector<unsigned long long> l(2 * n);
        for (uint64_t i = 0; i < n; ++i) l[2 * i] = add_lim[i], l[2 * i + 1] = rem_lim[i];
        JG_HIP(hipMemcpyAsync(d_lim, l.data(), 2 * n * 8, hipMemcpyHostToDevice, ctx->stream));
        JG_HIP(hipStreamSynchronize(ctx->stream));  // l is a local
    }
    jg::OrsetEncPlan& P = w->enc_plan;
    P.n = n;
    P.G = jg::orset_gather_sets(s, n, d_sets, d_lim, w->enc_g);
    const jg::OrsetGathered& G = P.G;
    const uint64_t R = G.R;
    const EncRec E{G.key, G.tlo, G.thi, G.ord, G.qs};
    // the encoder's arrays, one block
    const uint64_t R1 = R + 1;
    uint32_t *hf, *rend, *rfirst, *rval, *recv;
    ull *rkey, *cnt, *qlen, *reck, *reck2;
    unsigned* err;
    jg::Layout L;
    L.add(P.kidx, R), L.add(P.K, 1), L.add(hf, R), L.add(P.rid, R), L.add(P.rstart, R), L.add(rend, R), L.add(rfirst, R), L.add(P.nruns, 1);
    L.add(rkey, R), L.add(rval, R), L.add(P.skey, R), L.add(P.srun, R), L.add(P.rrank, R), L.add(cnt, R1), L.add(P.tlen, R1), L.add(P.rpos, R1), L.add(P.cpos, R1);
    L.add(P.qsec, 4 * n), L.add(P.sfirst, 4 * n), L.add(qlen, n + 1), L.add(P.qoff, n + 1);
    L.add(reck, R), L.add(recv, R), L.add(reck2, R), L.add(P.srec, R), L.add(P.rtags, R), L.add(err, 1);
    ensure(w->enc, L.bytes());
    L.bind(w->enc.p);
    JG_HIP(hipMemsetAsync(P.qsec, 0, 4 * n * 8, ctx->stream));
    JG_HIP(hipMemsetAsync(P.sfirst, 0xFF, 4 * n * 4, ctx->stream));
    JG_HIP(hipMemsetAsync(err, 0, 4, ctx->stream));
    JG_HIP(hipMemsetAsync(P.K, 0, 8, ctx->stream));
    JG_HIP(hipMemsetAsync(P.nruns, 0, 8, ctx->stream));
    const unsigned gR = blocks_for(R);
    if (R) {
        const int n_R = jg::cub_count(R, "records"), n_R1 = jg::cub_count(R1, "records");
        const auto tmp = jg::cub_in(w->cub);
        hipcub::CountingInputIterator<uint32_t> iota(0);
        jg::cub_run(tmp, [&](void* temp, size_t& bytes) { return hipcub::DeviceSelect::Flagged(temp, bytes, iota, G.keep, P.kidx, P.K, n_R, ctx->stream); });
        hipLaunchKernelGGL(k_enc_heads, dim3(gR), dim3(kBlock), 0, ctx->stream, E, P.kidx, P.K, R, hf);
        jg::cub_run(tmp, [&](void* temp, size_t& bytes) { return hipcub::DeviceScan::InclusiveSum(temp, bytes, hf, P.rid, n_R, ctx->stream); });
        hipLaunchKernelGGL(k_enc_runs, dim3(gR), dim3(kBlock), 0, ctx->stream, E, P.kidx, P.K, P.rid, P.rstart, rend, rfirst, P.nruns);
        hipLaunchKernelGGL(k_enc_first_ord, dim3(gR), dim3(kBlock), 0, ctx->stream, E, P.kidx, P.K, P.rid, rfirst);
        hipLaunchKernelGGL(k_enc_run_keys, dim3(gR), dim3(kBlock), 0, ctx->stream, E, P.kidx, P.rstart, rfirst, P.nruns, R, rkey, rval);
        JG_HIP(hipGetLastError());
        jg::cub_run(tmp, [&](void* temp, size_t& bytes) {
            return hipcub::DeviceRadixSort::SortPairs(temp, bytes, rkey, P.skey, rval, P.srun, n_R, 0, 64, ctx->stream);
        });
        hipLaunchKernelGGL(k_enc_run_len, dim3(gR), dim3(kBlock), 0, ctx->stream, E, N, P.kidx, P.rstart, rend, P.skey, P.srun, P.nruns, R, P.rrank, cnt,
                           P.tlen, P.qsec, P.sfirst, err);
        hipLaunchKernelGGL(k_enc_rec_keys, dim3(gR), dim3(kBlock), 0, ctx->stream, E, P.kidx, P.K, P.rid, P.rrank, R, reck, recv);
        JG_HIP(hipGetLastError());
        jg::cub_run(tmp, [&](void* temp, size_t& bytes) {
            return hipcub::DeviceRadixSort::SortPairs(temp, bytes, reck, reck2, recv, P.srec, n_R, 0, 64, ctx->stream);
        });
        JG_HIP(hipMemsetAsync(P.tlen + R, 0, 8, ctx->stream));
        JG_HIP(hipMemsetAsync(cnt + R, 0, 8, ctx->stream));
        jg::cub_run(tmp, [&](void* temp, size_t& bytes) { return hipcub::DeviceScan::ExclusiveSum(temp, bytes, P.tlen, P.rpos, n_R1, ctx->stream); });
        jg::cub_run(tmp, [&](void* temp, size_t& bytes) { return hipcub::DeviceScan::ExclusiveSum(temp, bytes, cnt, P.cpos, n_R1, ctx->stream); });
    }
    hipLaunchKernelGGL(k_enc_qlen, dim3(blocks_for(n + 1)), dim3(kBlock), 0, ctx->stream, P.qsec, n, qlen);
    JG_HIP(hipGetLastError());
    const int n_q = jg::cub_count(n + 1, "sets");
    jg::cub_run(jg::cub_in(w->cub), [&](void* temp, size_t& bytes) { return hipcub::DeviceScan::ExclusiveSum(temp, bytes, qlen, P.qoff, n_q, ctx->stream); });
    P.err = err;
}

// The write phase of the store's last size phase, at its offsets into dout (device; P.qoff[n] bytes).
void encode_write(jg_orset* s, uint8_t* dout) {
    jg_ctx* ctx = s->ctx;
    jg_orset_wire* w = s->wire;
    const Names N = w->names.view();
    const jg::OrsetEncPlan& P = w->enc_plan;
    const jg::OrsetGathered& G = P.G;
    const EncRec E{G.key, G.tlo, G.thi, G.ord, G.qs};
    const unsigned gR = blocks_for(G.R);
    hipLaunchKernelGGL(k_enc_fixed, dim3(blocks_for(P.n)), dim3(kBlock), 0, ctx->stream, P.qoff, P.qsec, P.n, dout);
    if (G.R) {
        hipLaunchKernelGGL(k_enc_run_text, dim3(gR), dim3(kBlock), 0, ctx->stream, E, N, P.kidx, P.rstart, P.skey, P.srun, P.nruns, P.rpos, P.tlen, P.sfirst,
                           P.qoff, P.qsec, P.rtags, dout);
        hipLaunchKernelGGL(k_enc_rec_text, dim3(gR), dim3(kBlock), 0, ctx->stream, E, P.kidx, P.K, P.srec, P.rid, P.rrank, P.cpos, P.rtags, dout);
    }
    JG_HIP(hipGetLastError());
}

void encode_sets(jg_orset* s, uint64_t n, const uint32_t* set, const uint64_t* add_lim, const uint64_t* rem_lim, uint64_t* off, uint8_t* out,
                 uint64_t cap, uint8_t* sha) {
    jg_ctx* ctx = s->ctx;
    encode_size(s, n, set, add_lim, rem_lim);
    const jg::OrsetEncPlan& P = s->wire->enc_plan;
    JG_HIP(hipMemcpyAsync(off, P.qoff, (n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    jg::pin_get(ctx, 0, P.err, 4);
    jg::pin_sync(ctx);  // the stream's copies above are done too
    unsigned e;
    std::memcpy(&e, jg::pin_at(ctx, 0), 4);
    JG_REQUIRE(e == 0, JG_ESTATE, "jg_orset_encode_json: a record names an element id the store's element table does not hold (names not synced)");
    if (!out) return;  // size query
    JG_REQUIRE(off[n] <= cap, JG_ESTATE, "jg_orset_encode_json: %llu bytes exceed cap %llu", (unsigned long long)off[n], (unsigned long long)cap);
    auto* dout = static_cast<uint8_t*>(jg::scratch(ctx, ctx->scratch2, off[n] + 64));
    encode_write(s, dout);
    if (sha) jg::sha256_device(ctx, dout, reinterpret_cast<const uint64_t*>(P.qoff), n, sha);  // each state's SHA-256 (ComputeDigest's first level)
    JG_HIP(hipMemcpyAsync(out, dout, off[n], hipMemcpyDeviceToHost, ctx->stream));
    JG_HIP(hipStreamSynchronize(ctx->stream));
}

}  // namespace

// jg_node_update_keys_ship (update.hip): the two phases with the offsets and the bytes left on the device
bool jg::orset_encode_size_locked(jg_orset* s, uint64_t n, const uint32_t* set, const uint64_t* add_lim, const uint64_t* rem_lim, uint64_t* h_off) {
    jg_ctx* ctx = s->ctx;
    encode_size(s, n, set, add_lim, rem_lim);
    const jg::OrsetEncPlan& P = s->wire->enc_plan;
    JG_HIP(hipMemcpyAsync(h_off, P.qoff, (n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    jg::pin_get(ctx, 0, P.err, 4);
    jg::pin_sync(ctx);
    unsigned e;
    std::memcpy(&e, jg::pin_at(ctx, 0), 4);
    return e == 0;
}

void jg::orset_encode_write_locked(jg_orset* s, uint8_t* d_out) { encode_write(s, d_out); }

extern "C" int jg_orset_encode_json(jg_orset* s, uint64_t n, const uint32_t* set, const uint64_t* add_lim, const uint64_t* rem_lim, uint64_t* off,
                                    uint8_t* out, uint64_t cap, uint8_t* sha) {
    return jg::guard([&] {
        auto lk_ = jg::lock(s);  // calls on one context are serialised (shared scratch, stream)
        JG_REQUIRE(s && off, JG_EINVAL, "jg_orset_encode_json: NULL argument");
        off[0] = 0;
        if (n == 0) return;
        JG_REQUIRE(set, JG_EINVAL, "jg_orset_encode_json: NULL set list");
        JG_REQUIRE(!add_lim == !rem_lim, JG_EINVAL, "jg_orset_encode_json: add_lim and rem_lim go together");
        JG_REQUIRE(n < (1ull << 29), JG_EINVAL, "jg_orset_encode_json: at most 2^29 states per call");
        jg::ensure_device(s->ctx);
        encode_sets(s, n, set, add_lim, rem_lim, off, out, cap, out ? sha : nullptr);
    });
}
