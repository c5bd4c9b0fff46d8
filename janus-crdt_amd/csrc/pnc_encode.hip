// pnc_encode.hip — everything that writes PNCounterMsg JSON or serves the producer: a store's rows encoded as the state
// messages the reference's nodes send (jg_pnc_encode_json, _before), and a batch of own-column client ops applied with
// the rewinds or the snapshots SafeCRDT.Update ships for them (jg_pnc_apply_ops_rewind, _encode).  json.hip reads them.
#include "pnc_table.hpp"
#include "snap_survivors.hpp"

namespace {

using jg::blocks_for;

// Increment / Decrement of one column (PNCounters.cs:97-112, unchecked '+='): wrapping atomic adds.
template <int EB>
__global__ __launch_bounds__(kBlock) void k_apply_ops_col(void* P, void* N, const uint32_t* __restrict__ key, uint32_t col,
                                                          const long long* __restrict__ delta, const uint8_t* __restrict__ is_n, uint64_t n,
                                                          uint32_t R) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t at = (uint64_t)key[i] * R + col;
    if constexpr (EB == 4) atomicAdd(static_cast<unsigned int*>(is_n[i] ? N : P) + at, (unsigned int)delta[i]);
    else atomicAdd(static_cast<unsigned long long*>(is_n[i] ? N : P) + at, (unsigned long long)delta[i]);
}

// ---- GetLastSynchronizedUpdate().Encode() on the device ----------------------
// PNCounterMsg.Encode (PNCounters.cs:46-49) of a row: {"pVector":{"<guid D>":P,...},"nVector":{...}}
// over the row's columns in table order (= the Dictionaries' enumeration order), System.Text.Json's
// compact form (the oracle's json::EncodePNC is the checker).  Pass 0: byte length per row; scan;
// pass 1: each thread writes its row's bytes.
__device__ __forceinline__ uint32_t dec_len(long long v) {
    unsigned long long u = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
    uint32_t n = v < 0 ? 2 : 1;
    while (u >= 10) { u /= 10; ++n; }
    return n;
}

template <int EB>
__device__ __forceinline__ long long cell(const void* base, uint64_t i) {
    if constexpr (EB == 4) return static_cast<const int*>(base)[i];
    else return static_cast<const long long*>(base)[i];
}

struct Out {
    uint8_t* p;
    __device__ void put(char c) { *p++ = (uint8_t)c; }
    template <int L>
    __device__ void str(const char (&s)[L]) {  // literals only: unrolled into immediate stores
#pragma unroll
        for (int k = 0; k + 1 < L; ++k) put(s[k]);
    }
    __device__ static char hexc(uint32_t v) {  // arithmetic, not a table: an indexed table is a memory load per digit
        v &= 15;
        return (char)(v < 10 ? '0' + v : 'a' - 10 + v);
    }
    __device__ void hex2(uint32_t b) {
        put(hexc(b >> 4));
        put(hexc(b));
    }
    __device__ void guid(const Guid16& g) {  // Guid.ToString("D"): b3b2b1b0-b5b4-b7b6-b8b9-b10..b15
        for (int k = 3; k >= 0; --k) hex2((uint32_t)(g.lo >> (8 * k)));
        put('-');
        hex2((uint32_t)(g.lo >> 40)); hex2((uint32_t)(g.lo >> 32));
        put('-');
        hex2((uint32_t)(g.lo >> 56)); hex2((uint32_t)(g.lo >> 48));
        put('-');
        hex2((uint32_t)g.hi); hex2((uint32_t)(g.hi >> 8));
        put('-');
        for (int k = 2; k < 8; ++k) hex2((uint32_t)(g.hi >> (8 * k)));
    }
    __device__ void dec(long long v) {
        char d[20];
        int n = 0;
        unsigned long long u = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
        do { d[n++] = (char)('0' + u % 10); u /= 10; } while (u);
        if (v < 0) put('-');
        while (n) put(d[--n]);
    }
};

// Rewind: the row as it stood before its last dp[i] / dn[i] of increments to column `col` (jg_pnc_encode_json_before;
// the cell type's wrapping arithmetic, as Increment's); NULL dp: the row as it is.
template <int EB>
__device__ __forceinline__ long long cell_at(const void* base, uint64_t i, bool rewind, long long d) {
    if constexpr (EB == 4) return rewind ? (long long)(int)((unsigned)cell<4>(base, i) - (unsigned)d) : cell<4>(base, i);
    else return rewind ? (long long)((unsigned long long)cell<8>(base, i) - (unsigned long long)d) : cell<8>(base, i);
}

template <int EB>
__device__ __forceinline__ void encode_row(Out o, Table t, const void* P, const void* N, uint32_t row, uint32_t col, bool rewind,
                                           long long rp, long long rn) {
    const uint32_t nc = t.ncols[row];
    const uint64_t base = (uint64_t)row * t.R;
    for (int which = 0; which < 2; ++which) {
        if (which) o.str("},\"nVector\":{");
        else o.str("{\"pVector\":{");
        const void* V = which ? N : P;
        for (uint32_t c = 0; c < nc; ++c) {
            if (c) o.put(',');
            o.put('"');
            o.guid(t.cols[base + c]);
            o.str("\":");
            o.dec(cell_at<EB>(V, base + c, rewind && c == col, which ? rn : rp));
        }
    }
    o.str("}}");
}

// The write pass stages each wave's rows in LDS.  A wave's rows are consecutive, so their states are one contiguous
// span of the output (the offsets are an exclusive scan), and the span goes out in aligned 16-byte stores of whole
// lines instead of every lane storing its own row a byte at a time ~370 bytes from its neighbours (64 partial lines
// per store instruction, which the memory side then merges line by line).  The span is placed in LDS at the output
// address's offset within 16 bytes, so LDS chunk k is output chunk k.  A span past kEncStage (rows with many replica
// columns) is written directly.  One wave per workgroup: 64 C5 rows (4 replicas) are ~23.5 KB.
constexpr uint32_t kEncStage = 32768;
constexpr int kEncLanes = 64;

template <int EB, int PASS>
__global__ __launch_bounds__(kBlock) void k_encode(const uint32_t* __restrict__ rows, uint64_t n, Table t, const void* P, const void* N,
                                                   unsigned long long* __restrict__ len_off, uint8_t* __restrict__ out, uint32_t col,
                                                   const long long* __restrict__ dp, const long long* __restrict__ dn) {
    if (PASS == 0) {
        const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
        if (i >= n) return;
        const uint32_t row = rows[i];
        const uint32_t nc = t.ncols[row];
        const uint64_t base = (uint64_t)row * t.R;
        const long long rp = dp ? dp[i] : 0, rn = dp ? dn[i] : 0;
        unsigned long long len = 27 + (nc ? 2ull * (40ull * nc - 1) : 0);
        for (uint32_t c = 0; c < nc; ++c)
            len += dec_len(cell_at<EB>(P, base + c, dp && c == col, rp)) + dec_len(cell_at<EB>(N, base + c, dp && c == col, rn));
        len_off[i] = len;
        return;
    } else {  // launched with kEncLanes threads per workgroup
        __shared__ __attribute__((aligned(16))) uint8_t stage[kEncStage + 16];
        const uint64_t first = (uint64_t)blockIdx.x * kEncLanes, i = first + threadIdx.x;
        const uint64_t last = first + kEncLanes < n ? first + kEncLanes : n;
        const unsigned long long lo = len_off[first], hi = len_off[last];  // (len_off holds n + 1 offsets)
        const bool staged = hi - lo <= kEncStage;  // uniform over the workgroup
        const uint32_t mis = (uint32_t)((uintptr_t)(out + lo) & 15);
        if (i < n) {
            const unsigned long long at = len_off[i];
            const uint32_t row = rows[i];
            const long long rp = dp ? dp[i] : 0, rn = dp ? dn[i] : 0;
            if (staged) encode_row<EB>(Out{stage + mis + (at - lo)}, t, P, N, row, col, dp != nullptr, rp, rn);  // LDS stores
            else encode_row<EB>(Out{out + at}, t, P, N, row, col, dp != nullptr, rp, rn);
        }
        if (!staged) return;
        __syncthreads();
        uint8_t* g = out + lo - mis;  // 16-byte aligned; only bytes [mis, end) of it are written
        const uint32_t end = mis + (uint32_t)(hi - lo), chunks = (end + 15) >> 4;
        for (uint32_t k = threadIdx.x; k < chunks; k += kEncLanes) {
            const uint32_t b0 = 16 * k;
            if (b0 >= mis && b0 + 16 <= end) {
                *reinterpret_cast<uint4*>(g + b0) = *reinterpret_cast<const uint4*>(stage + b0);
            } else {
                for (uint32_t b = b0; b < b0 + 16; ++b)
                    if (b >= mis && b < end) g[b] = stage[b];
            }
        }
    }
}

// ---- SafeCRDT.Update's rewinds on the device (jg_pnc_apply_ops_rewind) -------------------------------------------
// A batch of own-column client ops applied at once (PNCounters.cs:96-112), and for every op whose snapshot ships
// (SafeCRDT.cs:39-62), the amounts the batch's LATER ops on the same key added to P (Increment) and N (Decrement):
// jg_pnc_encode_json_before rewinds the row by them.  Keys are made in reverse op order and sorted stably on the row
// bits, so each key's ops sit together newest first, and an exclusive segmented sum over that order is exactly the
// later ops' amounts (wrapping, as the host's walk of round 5 summed them: 13-18 ms of host time per 1M C5 ops).
struct PN2 { unsigned long long p, n; };
struct PN2Add {
    __host__ __device__ PN2 operator()(const PN2& a, const PN2& b) const { return PN2{a.p + b.p, a.n + b.n}; }
};

// sorted position s: the op's amount on its vector (the store's width first, as the cells wrap), its key's row
__global__ void k_rewind_vals(const unsigned long long* __restrict__ sorted, uint64_t n, const long long* __restrict__ delta,
                              const uint8_t* __restrict__ is_n, uint32_t eb, PN2* __restrict__ vals, uint32_t* __restrict__ seg) {
    const uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n) return;
    const uint32_t i = (uint32_t)sorted[s];
    const unsigned long long a = (unsigned long long)(eb == 4 ? (long long)(int)delta[i] : delta[i]);
    vals[s] = is_n[i] ? PN2{0, a} : PN2{a, 0};
    seg[s] = (uint32_t)(sorted[s] >> 32);
}

__global__ void k_flags_u32(const uint8_t* __restrict__ f, uint64_t n, uint32_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = f[i] ? 1u : 0u;
}

// the needed ops' rewinds into need order (need_pos = exclusive count of needed ops before op i)
__global__ void k_rewind_scatter(const unsigned long long* __restrict__ sorted, uint64_t n, const PN2* __restrict__ later,
                                 const uint8_t* __restrict__ need, const uint32_t* __restrict__ need_pos, long long* __restrict__ dp,
                                 long long* __restrict__ dn) {
    const uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n) return;
    const uint32_t i = (uint32_t)sorted[s];
    if (!need[i]) return;
    dp[need_pos[i]] = (long long)later[s].p;
    dn[need_pos[i]] = (long long)later[s].n;
}

// op i's snapshot from the row as it stands BEFORE the batch (jg_pnc_apply_ops_encode): the key's ops up to and
// including i added to it, i.e. minus the rewind k_encode subtracts.  `excl` is the exclusive segmented sum over the
// stably sorted (forward) order, `vals` each op's own amount.
__global__ void k_prefix_scatter(const unsigned long long* __restrict__ sorted, uint64_t n, const PN2* __restrict__ vals,
                                 const PN2* __restrict__ excl, long long* __restrict__ dp, long long* __restrict__ dn) {
    const uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n) return;
    const uint32_t i = (uint32_t)sorted[s];
    dp[i] = (long long)(0ull - (excl[s].p + vals[s].p));
    dn[i] = (long long)(0ull - (excl[s].n + vals[s].n));
}

// One workspace for the per-key PN2 scan over n items and a sum of m Ts (the apply-ops calls run one after the other):
// sized before their arrays exist.
template <class T> size_t scans_temp_bytes(jg_ctx* ctx, int n, int m) {
    return std::max(jg::cub_temp_bytes([&](void* temp, size_t& bytes) {
                        return hipcub::DeviceScan::ExclusiveScanByKey(temp, bytes, (const uint32_t*)nullptr, (const PN2*)nullptr, (PN2*)nullptr, PN2Add(),
                                                                      PN2{0, 0}, n, hipcub::Equality(), ctx->stream);
                    }),
                    jg::cub_temp_bytes([&](void* temp, size_t& bytes) {
                        return hipcub::DeviceScan::ExclusiveSum(temp, bytes, (const T*)nullptr, (T*)nullptr, m, ctx->stream);
                    }));
}

struct DevOps { uint32_t* key; long long* delta; uint8_t* is_n; };  // a batch of ops on the device

// Increment / Decrement: every op added to column col of its key's row
void launch_apply_ops(jg_pnc* p, const DevOps& d, uint64_t n, uint32_t col) {
    jg::dispatch_eb(p->eb, [&](auto EB) {
        hipLaunchKernelGGL(k_apply_ops_col<EB()>, dim3(blocks_for(n)), dim3(kBlock), 0, p->ctx->stream, p->rw_P(), p->rw_N(), d.key, col, d.delta, d.is_n, n, p->R);
    });
    JG_HIP(hipGetLastError());
}

// An encode's arrays.  Device: the n rows, their rewinds (both or neither), room for n + 1 lengths and n + 1 offsets.
// Host: off [n + 1], out [cap] (NULL: the offsets only, a size query), sha [n x 32] or NULL.
struct Encode { const uint32_t* rows; const long long *dp, *dn; unsigned long long *len, *doff; uint64_t* off; uint8_t* out; uint64_t cap; uint8_t* sha; };

// The length pass: each entry's byte length, then the n + 1 offsets of an exclusive scan (e.doff, on the device).
// n1 = cub_count(n + 1), `tmp` the scan's workspace.
template <class Tmp>
void encode_lengths(jg_pnc* p, uint64_t n, int n1, uint32_t col, const Encode& e, Tmp&& tmp) {
    jg_ctx* ctx = p->ctx;
    const Table t = table_of(p);
    jg::dispatch_eb(p->eb, [&](auto EB) {
        hipLaunchKernelGGL((k_encode<EB(), 0>), dim3(blocks_for(n)), dim3(kBlock), 0, ctx->stream, e.rows, n, t, p->ro_P(), p->ro_N(), e.len, nullptr, col, e.dp, e.dn);
    });
    JG_HIP(hipGetLastError());
    JG_HIP(hipMemsetAsync(e.len + n, 0, 8, ctx->stream));
    jg::cub_run(tmp, [&](void* temp, size_t& bytes) { return hipcub::DeviceScan::ExclusiveSum(temp, bytes, e.len, e.doff, n1, ctx->stream); });
}

// The write pass at those offsets into dout (device): one wave per workgroup.
void encode_write(jg_pnc* p, uint64_t n, uint32_t col, const Encode& e, uint8_t* dout) {
    jg_ctx* ctx = p->ctx;
    const Table t = table_of(p);
    jg::dispatch_eb(p->eb, [&](auto EB) {
        hipLaunchKernelGGL((k_encode<EB(), 1>), dim3(blocks_for(n, kEncLanes)), dim3(kEncLanes), 0, ctx->stream, e.rows, n, t, p->ro_P(), p->ro_N(), e.doff, dout, col, e.dp, e.dn);
    });
    JG_HIP(hipGetLastError());
}

// The two-pass encode: lengths -> offsets on the host -> cap check (`cap_note`: what fn's error adds) -> bytes
// (ctx->scratch2), with their hashes if asked, to the host.  `ops` (or NULL) are applied behind the write pass and in
// front of the hashes and the copy: both passes read the rows before the adds land.
template <class Tmp>
void encode_two_pass(jg_pnc* p, uint64_t n, int n1, uint32_t col, const Encode& e, Tmp&& tmp, const char* fn, const char* cap_note, const DevOps* ops) {
    jg_ctx* ctx = p->ctx;
    encode_lengths(p, n, n1, col, e, tmp);
    JG_HIP(hipMemcpyAsync(e.off, e.doff, (n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    JG_HIP(hipStreamSynchronize(ctx->stream));
    if (!e.out) return;  // size query
    JG_REQUIRE(e.off[n] <= e.cap, JG_ESTATE, "%s: %llu bytes exceed cap %llu%s", fn, (unsigned long long)e.off[n], (unsigned long long)e.cap, cap_note);
    auto* dout = static_cast<uint8_t*>(jg::scratch(ctx, ctx->scratch2, e.off[n] + 64));
    encode_write(p, n, col, e, dout);
    if (ops) launch_apply_ops(p, *ops, n, col);
    if (e.sha) jg::sha256_device(ctx, dout, reinterpret_cast<const uint64_t*>(e.doff), n, e.sha);  // each state's SHA-256 (ComputeDigest's first level)
    JG_HIP(hipMemcpyAsync(e.out, dout, e.off[n], hipMemcpyDeviceToHost, ctx->stream));
    JG_HIP(hipStreamSynchronize(ctx->stream));
}

// jg_pnc_encode_json(_before): the rows and their rewinds uploaded, then the two passes.
void encode_rows(jg_pnc* p, uint64_t n, const uint32_t* key_idx, uint32_t col, const int64_t* dp, const int64_t* dn, uint64_t* off, uint8_t* out,
                 uint64_t cap, const char* fn, uint8_t* sha = nullptr) {
    JG_REQUIRE(p && off, JG_EINVAL, "%s: NULL argument", fn);
    off[0] = 0;
    if (n == 0) return;
    JG_REQUIRE(key_idx, JG_EINVAL, "%s: NULL key_idx", fn);
    JG_REQUIRE(n <= 0x7FFFFFFFull, JG_EINVAL, "%s: at most 2^31-1 rows per call", fn);
    for (uint64_t i = 0; i < n; ++i)
        JG_REQUIRE(key_idx[i] < p->n_keys, JG_EINVAL, "%s: key_idx[%llu] = %u out of range", fn, (unsigned long long)i, key_idx[i]);
    jg_ctx* ctx = p->ctx;
    jg::ensure_device(ctx);
    ensure_table(p);
    uint32_t* rows;
    unsigned long long *len, *doff;
    long long *ddp, *ddn;
    jg::Layout L;
    L.add(rows, n), L.add(len, n + 1), L.add(doff, n + 1, 8), L.add(ddp, dp ? n : 0, 8), L.add(ddn, dp ? n : 0, 8);
    L.bind(jg::scratch(ctx, ctx->scratch, L.bytes() + 256));
    if (!dp) ddp = ddn = nullptr;
    JG_HIP(hipMemcpyAsync(rows, key_idx, n * 4, hipMemcpyHostToDevice, ctx->stream));
    if (dp) {
        JG_HIP(hipMemcpyAsync(ddp, dp, n * 8, hipMemcpyHostToDevice, ctx->stream));
        JG_HIP(hipMemcpyAsync(ddn, dn, n * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    encode_two_pass(p, n, jg::cub_count(n + 1, "rows"), col, Encode{rows, ddp, ddn, len, doff, off, out, cap, sha}, jg::cub_in(ctx, ctx->scratch3), fn, "",
                    nullptr);
}

// What both apply-ops calls check of their ops (`args`: the call's own pointers are all there) ...
void check_ops(const jg_pnc* p, const char* fn, uint64_t n, const uint32_t* key, uint32_t col, bool args) {
    JG_REQUIRE(args, JG_EINVAL, "%s: NULL argument", fn);
    JG_REQUIRE(col < p->R, JG_EINVAL, "%s: column %u past the store's %u replicas", fn, col, p->R);
    JG_REQUIRE(n <= 0x7FFFFFFFull, JG_EINVAL, "%s: at most 2^31-1 ops per call", fn);
    for (uint64_t i = 0; i < n; ++i)
        JG_REQUIRE(key[i] < p->n_keys, JG_EINVAL, "%s: op %llu addresses key %u outside the store", fn, (unsigned long long)i, key[i]);
}

// ... and how they upload them, into arrays the call carved itself
void upload_ops(jg_ctx* ctx, const DevOps& d, uint64_t n, const uint32_t* key, const int64_t* delta, const uint8_t* is_n) {
    JG_HIP(hipMemcpyAsync(d.key, key, n * 4, hipMemcpyHostToDevice, ctx->stream));
    JG_HIP(hipMemcpyAsync(d.delta, delta, n * 8, hipMemcpyHostToDevice, ctx->stream));
    JG_HIP(hipMemcpyAsync(d.is_n, is_n, n, hipMemcpyHostToDevice, ctx->stream));
}

// Per key, each op's amounts (vals) and the sum of the amounts ahead of it in its key's run (sums): keys in op order,
// or (REV) newest first -> stable sort on the row -> amounts -> exclusive scan by key.  Returns the sorted keys
// (sort_keys: ctx->scratch3); vals, sums and seg are in sorted order.  n_rows: the rows the sort tells apart (the store's,
// or one more where d.key marks an entry that addresses no row with the store's n_keys: those sort to the end).
template <bool REV, class Tmp>
const unsigned long long* key_amounts(jg_pnc* p, const DevOps& d, uint64_t n, uint64_t n_rows, unsigned long long* keys, PN2* vals, PN2* sums, uint32_t* seg,
                                      Tmp&& tmp) {
    jg_ctx* ctx = p->ctx;
    const unsigned g = blocks_for(n);
    const int n_i = jg::cub_count(n, "ops");
    hipLaunchKernelGGL(k_make_keys<REV>, dim3(g), dim3(kBlock), 0, ctx->stream, d.key, n, keys);
    JG_HIP(hipGetLastError());
    const unsigned long long* sorted = sort_keys(ctx, keys, n, n_rows);
    hipLaunchKernelGGL(k_rewind_vals, dim3(g), dim3(kBlock), 0, ctx->stream, sorted, n, d.delta, d.is_n, p->eb, vals, seg);
    JG_HIP(hipGetLastError());
    jg::cub_run(tmp, [&](void* temp, size_t& bytes) {
        return hipcub::DeviceScan::ExclusiveScanByKey(temp, bytes, seg, vals, sums, PN2Add(), PN2{0, 0}, n_i, hipcub::Equality(), ctx->stream);
    });
    return sorted;
}

// ---- the snapshots of a batch resolved on the device (jg_node_update_keys_encode) -----------------
// The batch is sorted with the commands that apply no PN-Counter op under row `none_row` (the store's n_keys), behind
// every real row; who ships is snap_survivors.hpp's rule over the row.

// sorted position s: its object key (jg_node_update_keys_ship's OR-Set commands, keyed by set id)
__global__ void k_obj_seg(const unsigned long long* __restrict__ sorted, uint64_t n, uint32_t* __restrict__ seg) {
    const uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s < n) seg[s] = (uint32_t)(sorted[s] >> 32);
}

// the encode list: the taken commands' rows and rewinds at their positions (pos = exclusive count of taken commands)
__global__ void k_snap_list(const uint32_t* __restrict__ take, const uint32_t* __restrict__ pos, uint64_t n, const uint32_t* __restrict__ row,
                            const long long* __restrict__ dp, const long long* __restrict__ dn, uint32_t* __restrict__ erow,
                            long long* __restrict__ edp, long long* __restrict__ edn) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || !take[i]) return;
    const uint32_t j = pos[i];
    erow[j] = row[i], edp[j] = dp[i], edn[j] = dn[i];
}

// the list's offsets back by command index: command i's bytes begin where list entry pos[i] begins (i = n: the total)
__global__ void k_snap_offsets(const uint32_t* __restrict__ pos, uint64_t n, const unsigned long long* __restrict__ eoff,
                               unsigned long long* __restrict__ snap_off) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i <= n) snap_off[i] = eoff[pos[i]];
}

}  // namespace

namespace jg {

void pnc_snap_plan_locked(jg_pnc* p, const PncSnap& s, uint64_t n, uint32_t col, uint64_t* m_out, uint64_t* h_snap_off, hipEvent_t* ev) {
    jg_ctx* ctx = p->ctx;
    const auto stamp = [&](int k) {
        if (ev) JG_HIP(hipEventRecord(ev[k], ctx->stream));
    };
    JG_REQUIRE(col < p->R, JG_EINVAL, "pnc_snap_plan: column %u past the store's %u replicas", col, p->R);
    JG_REQUIRE(p->n_keys < 0xFFFFFFFFull, JG_EINVAL, "pnc_snap_plan: the store's %llu rows leave no row id free", (unsigned long long)p->n_keys);
    ensure_table(p);
    const uint32_t none_row = (uint32_t)p->n_keys;
    const int n_i = jg::cub_count(n, "commands"), n1_i = jg::cub_count(n + 1, "commands");
    const size_t t_all = std::max({scans_temp_bytes<unsigned long long>(ctx, n_i, n1_i), scans_temp_bytes<uint32_t>(ctx, n_i, n1_i),
                                   jg::cub_temp_bytes([&](void* temp, size_t& bytes) {
                                       return hipcub::DeviceScan::InclusiveScan(temp, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, hipcub::Max(), n_i,
                                                                                ctx->stream);
                                   })});
    // everything that does not outlive this step in ctx->scratch; the sort in scratch3
    uint32_t *seg, *mark, *head, *latest, *take, *pos;
    long long *ddp, *ddn;
    unsigned long long *keys, *len;
    PN2 *vals, *excl;
    uint8_t* dtmp;
    jg::Layout A;
    A.add(keys, n), A.add(vals, n), A.add(excl, n), A.add(seg, n), A.add(mark, n), A.add(head, n), A.add(latest, n), A.add(take, n + 1), A.add(pos, n + 1);
    if (!s.pdp) A.add(ddp, n), A.add(ddn, n);
    A.add(len, n + 1), A.add(dtmp, t_all + 256);
    A.bind(jg::scratch(ctx, ctx->scratch, A.bytes()));
    if (s.pdp) ddp = s.pdp, ddn = s.pdn;  // kept by the caller for the batch's reads
    const auto tmp = jg::cub_in(dtmp, t_all);
    const unsigned g = blocks_for(n);
    // each command's amounts up to and including it on its row, in batch order (the commands without a row add 0 to a
    // run of their own)
    const DevOps d{const_cast<uint32_t*>(s.row), const_cast<long long*>(s.amount), const_cast<uint8_t*>(s.is_n)};
    const unsigned long long* sorted = key_amounts<false>(p, d, n, p->n_keys + 1, keys, vals, excl, seg, tmp);
    hipLaunchKernelGGL(k_prefix_scatter, dim3(g), dim3(kBlock), 0, ctx->stream, sorted, n, vals, excl, ddp, ddn);
    // the survivors of snap == 2, then who ships a snapshot
    snap_survivors(ctx, sorted, seg, n, n_i, none_row, s.snap, mark, head, latest, s.none, take, tmp);
    JG_HIP(hipMemsetAsync(take + n, 0, 4, ctx->stream));
    jg::cub_run(tmp, [&](void* temp, size_t& bytes) { return hipcub::DeviceScan::ExclusiveSum(temp, bytes, take, pos, n1_i, ctx->stream); });
    hipLaunchKernelGGL(k_snap_list, dim3(g), dim3(kBlock), 0, ctx->stream, take, pos, n, s.row, ddp, ddn, s.erow, s.edp, s.edn);
    JG_HIP(hipGetLastError());
    stamp(0);
    jg::pin_get(ctx, 0, pos + n, 4);
    jg::pin_sync(ctx);
    const uint64_t m = *static_cast<const uint32_t*>(jg::pin_at(ctx, 0));
    *m_out = m;
    if (m == 0) {
        JG_HIP(hipMemsetAsync(s.snap_off, 0, (n + 1) * 8, ctx->stream));
        std::fill(h_snap_off, h_snap_off + n + 1, 0);
        stamp(1);
        return;
    }
    // the list's lengths and offsets (nothing is applied yet), and the offsets by command index to the host
    encode_lengths(p, m, jg::cub_count(m + 1, "commands"), col, Encode{s.erow, s.edp, s.edn, len, s.eoff, nullptr, nullptr, 0, nullptr}, tmp);
    hipLaunchKernelGGL(k_snap_offsets, dim3(blocks_for(n + 1)), dim3(kBlock), 0, ctx->stream, pos, n, s.eoff, s.snap_off);
    JG_HIP(hipGetLastError());
    stamp(1);
    JG_HIP(hipMemcpyAsync(h_snap_off, s.snap_off, (n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    JG_HIP(hipStreamSynchronize(ctx->stream));
}

const uint8_t* pnc_snap_bytes_locked(jg_pnc* p, const PncSnap& s, uint64_t m, uint64_t bytes, uint32_t col) {
    jg_ctx* ctx = p->ctx;
    auto* dout = static_cast<uint8_t*>(jg::scratch(ctx, ctx->scratch2, bytes + 64));
    encode_write(p, m, col, Encode{s.erow, s.edp, s.edn, nullptr, s.eoff, nullptr, nullptr, 0, nullptr}, dout);
    return dout;
}

void snap_survivors_locked(jg_ctx* ctx, const uint32_t* d_obj, uint64_t n, uint32_t none_obj, const uint8_t* d_snap, uint8_t* d_none) {
    const int n_i = jg::cub_count(n, "commands");
    const size_t t_scan = jg::cub_temp_bytes([&](void* temp, size_t& bytes) {
        return hipcub::DeviceScan::InclusiveScan(temp, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, hipcub::Max(), n_i, ctx->stream);
    });
    unsigned long long* keys;
    uint32_t *seg, *mark, *head, *latest, *take;
    uint8_t* dtmp;
    jg::Layout A;
    A.add(keys, n), A.add(seg, n), A.add(mark, n), A.add(head, n), A.add(latest, n), A.add(take, n), A.add(dtmp, t_scan + 256);
    A.bind(jg::scratch(ctx, ctx->scratch, A.bytes()));
    const unsigned g = blocks_for(n);
    hipLaunchKernelGGL(k_make_keys<false>, dim3(g), dim3(kBlock), 0, ctx->stream, d_obj, n, keys);
    JG_HIP(hipGetLastError());
    const unsigned long long* sorted = sort_keys(ctx, keys, n, (uint64_t)none_obj + 1);
    hipLaunchKernelGGL(k_obj_seg, dim3(g), dim3(kBlock), 0, ctx->stream, sorted, n, seg);
    snap_survivors(ctx, sorted, seg, n, n_i, none_obj, d_snap, mark, head, latest, d_none, take, jg::cub_in(dtmp, t_scan));
}

void pnc_snap_write_locked(jg_pnc* p, const PncSnap& s, uint64_t n, uint64_t m, uint64_t bytes, uint32_t col, uint8_t* out, uint8_t* sha,
                           hipEvent_t* ev) {
    jg_ctx* ctx = p->ctx;
    const auto stamp = [&](int k) {
        if (ev) JG_HIP(hipEventRecord(ev[k], ctx->stream));
    };
    if (m == 0) {
        if (sha) std::memset(sha, 0, n * 32);
        for (int k = 2; k < 5; ++k) stamp(k);
        return;
    }
    const uint8_t* dout = pnc_snap_bytes_locked(p, s, m, bytes, col);
    stamp(2);
    if (sha) jg::sha256_device(ctx, dout, reinterpret_cast<const uint64_t*>(s.snap_off), n, sha, s.none);
    stamp(3);
    JG_HIP(hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, ctx->stream));
    stamp(4);
}

}  // namespace jg

extern "C" {

int jg_pnc_apply_ops_rewind(jg_pnc* p, uint64_t n_ops, const uint32_t* key, uint32_t col, const int64_t* delta, const uint8_t* is_n,
                            const uint8_t* need, int64_t* dp, int64_t* dn) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        jg::require_writable(p, "jg_pnc_apply_ops_rewind");
        JG_REQUIRE(p, JG_EINVAL, "jg_pnc_apply_ops_rewind: store is NULL");
        if (n_ops == 0) return;
        check_ops(p, "jg_pnc_apply_ops_rewind", n_ops, key, col, key && delta && is_n && need && dp && dn);
        const uint64_t n = n_ops;
        uint64_t n_need = 0;
        for (uint64_t i = 0; i < n; ++i) n_need += need[i] != 0;
        jg_ctx* ctx = p->ctx;
        jg::ensure_device(ctx);
        const int n_i = jg::cub_count(n, "ops");
        // the ops (scratch2): key, delta, is_n, need, then the need positions
        DevOps d;
        uint32_t* dpos;
        uint8_t* dneed;
        jg::Layout A;
        A.add(d.key, n), A.add(d.delta, n), A.add(d.is_n, n), A.add(dneed, n), A.add(dpos, n);
        A.bind(jg::scratch(ctx, ctx->scratch2, A.bytes() + 256));
        upload_ops(ctx, d, n, key, delta, is_n);
        JG_HIP(hipMemcpyAsync(dneed, need, n, hipMemcpyHostToDevice, ctx->stream));
        launch_apply_ops(p, d, n, col);
        if (n_need == 0) {
            JG_HIP(hipStreamSynchronize(ctx->stream));
            return;
        }
        // the rewinds (scratch: keys, values, sums, segments, the scans' temp; sort_keys uses scratch3)
        const size_t t_both = scans_temp_bytes<uint32_t>(ctx, n_i, n_i);
        unsigned long long* keys;
        PN2 *vals, *later;
        uint32_t* seg;
        long long* ddp;
        uint8_t* dtmp;
        jg::Layout B;
        B.add(keys, n), B.add(vals, n), B.add(later, n), B.add(seg, n), B.add(ddp, 2 * n_need), B.add(dtmp, t_both + 256);
        B.bind(jg::scratch(ctx, ctx->scratch, B.bytes()));
        long long* ddn = ddp + n_need;
        const auto tmp = jg::cub_in(dtmp, t_both);
        // need positions first (the flags as u32 in `seg`: a scan of u8 would sum in u8), then the later ops' amounts
        const unsigned g = blocks_for(n);
        hipLaunchKernelGGL(k_flags_u32, dim3(g), dim3(kBlock), 0, ctx->stream, dneed, n, seg);
        jg::cub_run(tmp, [&](void* temp, size_t& bytes) { return hipcub::DeviceScan::ExclusiveSum(temp, bytes, seg, dpos, n_i, ctx->stream); });
        const unsigned long long* sorted = key_amounts<true>(p, d, n, p->n_keys, keys, vals, later, seg, tmp);
        hipLaunchKernelGGL(k_rewind_scatter, dim3(g), dim3(kBlock), 0, ctx->stream, sorted, n, later, dneed, dpos, ddp, ddn);
        JG_HIP(hipGetLastError());
        JG_HIP(hipMemcpyAsync(dp, ddp, n_need * 8, hipMemcpyDeviceToHost, ctx->stream));
        JG_HIP(hipMemcpyAsync(dn, ddn, n_need * 8, hipMemcpyDeviceToHost, ctx->stream));
        JG_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int jg_pnc_apply_ops_encode(jg_pnc* p, uint64_t n_ops, const uint32_t* key, uint32_t col, const int64_t* delta, const uint8_t* is_n,
                            uint64_t* off, uint8_t* out, uint64_t cap, uint8_t* sha) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        JG_REQUIRE(p && off, JG_EINVAL, "jg_pnc_apply_ops_encode: NULL argument");
        jg::require_writable(p, "jg_pnc_apply_ops_encode");
        off[0] = 0;
        if (n_ops == 0) return;
        check_ops(p, "jg_pnc_apply_ops_encode", n_ops, key, col, key && delta && is_n && out);
        jg_ctx* ctx = p->ctx;
        jg::ensure_device(ctx);
        ensure_table(p);
        const uint64_t n = n_ops;
        const int n1_i = jg::cub_count(n + 1, "ops");
        const size_t t_both = scans_temp_bytes<unsigned long long>(ctx, jg::cub_count(n, "ops"), n1_i);
        // everything but the sort (scratch3) and the bytes (scratch2) in ctx->scratch
        DevOps d;
        uint32_t* seg;
        long long *ddp, *ddn;
        uint8_t* dtmp;
        unsigned long long *keys, *len, *doff;
        PN2 *vals, *excl;
        jg::Layout A;
        A.add(d.key, n), A.add(d.delta, n), A.add(d.is_n, n), A.add(keys, n), A.add(vals, n), A.add(excl, n), A.add(seg, n), A.add(ddp, n), A.add(ddn, n);
        A.add(len, n + 1), A.add(doff, n + 1), A.add(dtmp, t_both + 256);
        A.bind(jg::scratch(ctx, ctx->scratch, A.bytes()));
        const auto tmp = jg::cub_in(dtmp, t_both);
        upload_ops(ctx, d, n, key, delta, is_n);
        // each op's amounts up to and including it, per key (forward keys: a stable sort keeps op order per key)
        const unsigned long long* sorted = key_amounts<false>(p, d, n, p->n_keys, keys, vals, excl, seg, tmp);
        hipLaunchKernelGGL(k_prefix_scatter, dim3(blocks_for(n)), dim3(kBlock), 0, ctx->stream, sorted, n, vals, excl, ddp, ddn);
        JG_HIP(hipGetLastError());
        // the snapshots from the rows as they stand (nothing applied yet), then the ops
        encode_two_pass(p, n, n1_i, col, Encode{d.key, ddp, ddn, len, doff, off, out, cap, sha}, tmp, "jg_pnc_apply_ops_encode", " (nothing applied)", &d);
    });
}

int jg_pnc_encode_json(jg_pnc* p, uint64_t n, const uint32_t* key_idx, uint64_t* off, uint8_t* out, uint64_t cap) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        encode_rows(p, n, key_idx, 0, nullptr, nullptr, off, out, cap, "jg_pnc_encode_json");
    });
}

int jg_pnc_encode_json_before(jg_pnc* p, uint64_t n, const uint32_t* key_idx, uint32_t col, const int64_t* dp, const int64_t* dn, uint64_t* off,
                              uint8_t* out, uint64_t cap, uint8_t* sha) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);
        JG_REQUIRE(p && (n == 0 || (dp && dn)), JG_EINVAL, "jg_pnc_encode_json_before: NULL argument");
        JG_REQUIRE(col < p->R, JG_EINVAL, "jg_pnc_encode_json_before: column %u past the store's %u replicas", col, p->R);
        encode_rows(p, n, key_idx, col, dp, dn, off, out, cap, "jg_pnc_encode_json_before", out ? sha : nullptr);
    });
}

}  // extern "C"

