// pnc.hip — PN-Counter store and kernels (gfx950, wave64, no MFMA: integer bandwidth work).
//
// Layout in HBM: P and N are row-major [n_keys x R] arrays of the store's width (int32 = the
// reference's `int`, int64 = the BASELINE variant).  Row = interned key, column = interned replica.
//
// The dense identity merge (jg::pnc_merge_dense, its shadow, the received batch's handle) is csrc/pnc_dense.hip's.
// Kernels and their roofline (HBM):
//   k_merge_indexed  scatter-max of received rows into their keys (atomicMax: rows may repeat a
//                    key inside one committed batch, SafeCRDTManager.cs:122-146).
//   k_apply_ops      Increment/Decrement (PNCounters.cs:97-112): wrapping atomic adds.
//   k_values         PNCounter.Get (PNCounters.cs:87-90): one wave per key, exact prefix sums in
//                    column order to reproduce the checked LINQ Sum's OverflowException.
//   k_restride       jg_pnc_reserve's widening: dst[k][0..R_old) = src[k][0..R_old), zero elsewhere (a row
//                    the Dictionary<Guid,int> grows into, PNCounters.cs:131-144).  Reads the old bytes once,
//                    writes the new bytes once: (old + new) bytes at HBM rate.
#include <algorithm>
#include <cstdlib>

#include "launch.hpp"
#include "pnc_vec.hpp"

namespace {

using jg::check_store;
using namespace jg::filt;  // pnc_vec.hpp: nt_ld / nt_st, vmax, differs, group_any and kElideLanes

constexpr int kBlock = 256;

template <int EB> struct Elem;
template <> struct Elem<4> { using T = int; };
template <> struct Elem<8> { using T = long long; };

// Scatter-max: cell (m, c) of the received rows into row keys[m].  ABSENT cells are skipped.
template <int EB>
__global__ __launch_bounds__(kBlock) void k_merge_indexed(typename Elem<EB>::T* __restrict__ AP, typename Elem<EB>::T* __restrict__ AN,
                                                          const typename Elem<EB>::T* __restrict__ BP,
                                                          const typename Elem<EB>::T* __restrict__ BN,
                                                          const uint32_t* __restrict__ keys, uint64_t n_rows, uint32_t R) {
    using T = typename Elem<EB>::T;
    const T absent = EB == 4 ? (T)INT32_MIN : (T)INT64_MIN;
    const uint64_t n = n_rows * R;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const uint64_t m = i / R, c = i - m * R;
        const uint64_t at = (uint64_t)keys[m] * R + c;
        const T p = BP[i], q = BN[i];
        if (p != absent) atomicMax(AP + at, p);
        if (q != absent) atomicMax(AN + at, q);
    }
}

// The same scatter-max with one wave per received row (lanes over columns): no 64-bit division per
// cell, coalesced row loads and row-contiguous atomics.  Used when a row fills most of a wave (R >= 32).
template <int EB>
__global__ __launch_bounds__(kBlock) void k_merge_indexed_rows(typename Elem<EB>::T* __restrict__ AP, typename Elem<EB>::T* __restrict__ AN,
                                                               const typename Elem<EB>::T* __restrict__ BP,
                                                               const typename Elem<EB>::T* __restrict__ BN,
                                                               const uint32_t* __restrict__ keys, uint64_t n_rows, uint32_t R) {
    using T = typename Elem<EB>::T;
    const T absent = EB == 4 ? (T)INT32_MIN : (T)INT64_MIN;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t n_waves = ((uint64_t)gridDim.x * kBlock) >> 6;
    for (uint64_t m = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6; m < n_rows; m += n_waves) {
        const uint64_t at = (uint64_t)keys[m] * R, src = m * R;
        for (uint32_t c = lane; c < R; c += 64) {
            const T p = BP[src + c], q = BN[src + c];
            if (p != absent) atomicMax(AP + at + c, p);
            if (q != absent) atomicMax(AN + at + c, q);
        }
    }
}

// Duplicate-aware scatter-max with no atomics on the data, two passes over the batch's keys (a committed
// wave folds several states of one key, SafeCRDTManager.cs:122-146).  Pass 1 (k_group_link) links each
// key's rows into a list: next[m] = the key's previous head, head[key] = gen << 32 | m (one atomicExch per
// row).  Pass 2 (k_merge_grouped): the head row of every key loads its A row once, max-folds every B row of
// the key in registers — each B row's load issued together with its next[] link, so a key held k times
// costs k - 1 dependent hops — and stores the 128-B lines of A that the fold raised, once (store elision, group_any:
// a key whose rows are all at or below A writes nothing); the other rows of the key do nothing.  Heads carry the
// batch's generation: a head left by an earlier batch reads as empty, so nothing resets them (the list
// head's `head[key] = kNil` store was one more random write per distinct key: 0.578 -> 0.566 ms per 1M rows,
// tools/tune_grouped.hip).  Atomics ran at ~1.3 TB/s of added bytes on MI355X against ~6 TB/s for plain
// stores (MI355X_MICROARCH.md, atomics table), and random 4-B atomics ~17x slower again: a per-cell
// atomicMax for repeated keys (39 % of the rows of a uniform batch of n rows over 2n keys) and an
// occurrence count per row both measured slower (tools/tune_grouped.hip).  ABSENT (the
// width's minimum) needs no test: max(a, ABSENT) = a.
constexpr uint32_t kNil = 0xFFFFFFFFu;

__global__ __launch_bounds__(kBlock) void k_group_link(const uint32_t* __restrict__ keys, uint64_t n, unsigned long long* __restrict__ head,
                                                       uint32_t* __restrict__ next, unsigned long long gen) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const unsigned long long old = atomicExch(head + keys[i], gen << 32 | i);
        next[i] = (old >> 32) == gen ? (uint32_t)old : kNil;
    }
}

// One wave per received row, U rows in flight; the row (R x EB bytes) is a whole number of 16-B vectors
// and each lane owns the same vector slot(s) of every row it touches.
template <int EB, int U>
__global__ __launch_bounds__(kBlock) void k_merge_grouped(typename Elem<EB>::T* __restrict__ AP, typename Elem<EB>::T* __restrict__ AN,
                                                          const typename Elem<EB>::T* __restrict__ BP,
                                                          const typename Elem<EB>::T* __restrict__ BN, const uint32_t* __restrict__ keys,
                                                          const unsigned long long* __restrict__ head, const uint32_t* __restrict__ next,
                                                          uint64_t n_rows, uint32_t R, unsigned long long gen) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t nv = R * EB / 16;  // vectors per array row
    const uint64_t n_waves = ((uint64_t)gridDim.x * kBlock) >> 6;
    for (uint64_t m0 = (((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6) * U; m0 < n_rows; m0 += n_waves * U) {
        uint64_t key[U];
        bool lead[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t m = m0 + u;
            key[u] = m < n_rows ? keys[m] : 0;
            lead[u] = m < n_rows && head[key[u]] == (gen << 32 | m);
        }
        for (uint32_t v = lane; v < 2 * nv; v += 64) {
            const bool isP = v < nv;
            const uint32_t w = isP ? v : v - nv;
            const auto* B = isP ? BP : BN;
            auto* A = isP ? AP : AN;
            uint4 a[U], a0[U], b[U];  // a0: the A vector as loaded (store elision)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (lead[u]) {
                    b[u] = nt_ld(reinterpret_cast<const uint4*>(B + (m0 + u) * R) + w);
                    a0[u] = *(reinterpret_cast<const uint4*>(A + key[u] * R) + w);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!lead[u]) continue;
                a[u] = vmax<EB>(a0[u], b[u]);
                uint64_t hops = 0;  // a list holds at most n_rows - 1 more rows: a bound every walk reaches
                for (uint32_t cur = next[m0 + u]; cur != kNil && ++hops < n_rows;) {  // the key's other rows
                    const uint4 bb = nt_ld(reinterpret_cast<const uint4*>(B + (uint64_t)cur * R) + w);
                    const uint32_t nx = next[cur];
                    a[u] = vmax<EB>(a[u], bb);
                    cur = nx;
                }
                // lead[u] and the list walk are wave-uniform: the ballot is taken by the lanes of this trip of the
                // v loop (the last trip's idle lanes vote unchanged)
                if (group_any<kElideLanes>(__ballot(differs(a[u], a0[u])), lane)) *(reinterpret_cast<uint4*>(A + key[u] * R) + w) = a[u];
            }
        }
    }
}

// Row copy (write: keys on the destination side; read: keys on the source side).
template <int EB>
__global__ __launch_bounds__(kBlock) void k_rows_copy(typename Elem<EB>::T* __restrict__ dst, const typename Elem<EB>::T* __restrict__ src,
                                                      const uint32_t* __restrict__ keys, uint64_t n_rows, uint32_t R, int scatter) {
    const uint64_t n = n_rows * R;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const uint64_t m = i / R, c = i - m * R;
        const uint64_t at = (uint64_t)keys[m] * R + c;
        if (scatter) dst[at] = src[i];
        else dst[i] = src[at];
    }
}

// Increment / Decrement: unchecked '+=' == wrapping add; order-free, so atomics are exact.
template <int EB>
__global__ __launch_bounds__(kBlock) void k_apply_ops(typename Elem<EB>::T* __restrict__ P, typename Elem<EB>::T* __restrict__ N,
                                                      const uint32_t* __restrict__ key, const uint32_t* __restrict__ col,
                                                      const long long* __restrict__ delta, const uint8_t* __restrict__ is_n,
                                                      uint64_t n_ops, uint32_t R) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n_ops; i += (uint64_t)gridDim.x * kBlock) {
        const uint64_t at = (uint64_t)key[i] * R + col[i];
        auto* base = is_n[i] ? N : P;
        if constexpr (EB == 4) atomicAdd(reinterpret_cast<unsigned int*>(base + at), (unsigned int)delta[i]);
        else atomicAdd(reinterpret_cast<unsigned long long*>(base + at), (unsigned long long)delta[i]);
    }
}

// The same adds over a device list of (row, amount, P | N) on one column (update.hip): the list's length is read from
// device memory, so the grid is fixed by the batch and no count visits the host.  The rows were checked against the
// store by the kernel that wrote the list, the column by the host.
template <int EB>
__global__ __launch_bounds__(kBlock) void k_add_list(typename Elem<EB>::T* __restrict__ P, typename Elem<EB>::T* __restrict__ N,
                                                     const uint32_t* __restrict__ row, const long long* __restrict__ amount,
                                                     const uint8_t* __restrict__ is_n, const unsigned long long* __restrict__ count, uint64_t n_max,
                                                     uint32_t col, uint32_t R) {
    const uint64_t n = *count < n_max ? *count : n_max;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const uint64_t at = (uint64_t)row[i] * R + col;
        auto* base = is_n[i] ? N : P;
        if constexpr (EB == 4) atomicAdd(reinterpret_cast<unsigned int*>(base + at), (unsigned int)amount[i]);
        else atomicAdd(reinterpret_cast<unsigned long long*>(base + at), (unsigned long long)amount[i]);
    }
}

// ---- PNCounter.Get: checked Sum in column order -------------------------------------------------
template <int EB> struct Acc;
template <> struct Acc<4> { using T = long long; };  // 64 x 2^31 fits easily
template <> struct Acc<8> { using T = __int128; };   // exact for any 64-bit prefix

__device__ __forceinline__ long long shfl_up_acc(long long v, int d) { return __shfl_up(v, d, 64); }
__device__ __forceinline__ __int128 shfl_up_acc(__int128 v, int d) {
    long long lo = (long long)v, hi = (long long)(v >> 64);
    lo = __shfl_up(lo, d, 64);
    hi = __shfl_up(hi, d, 64);
    return ((__int128)hi << 64) | (unsigned long long)lo;
}
__device__ __forceinline__ long long shfl_acc(long long v, int src) { return __shfl(v, src, 64); }
__device__ __forceinline__ __int128 shfl_acc(__int128 v, int src) {
    long long lo = (long long)v, hi = (long long)(v >> 64);
    lo = __shfl(lo, src, 64);
    hi = __shfl(hi, src, 64);
    return ((__int128)hi << 64) | (unsigned long long)lo;
}

// Returns the exact sum of cell(0) .. cell(R - 1); sets `of` if any prefix leaves T's range.
template <int EB, class Cell>
__device__ __forceinline__ typename Acc<EB>::T checked_sum_of(Cell cell, uint32_t R, int lane, bool& of) {
    using T = typename Elem<EB>::T;
    using A = typename Acc<EB>::T;
    const A lo = EB == 4 ? (A)INT32_MIN : (A)INT64_MIN;
    const A hi = EB == 4 ? (A)INT32_MAX : (A)INT64_MAX;
    A carry = 0;
    for (uint32_t c0 = 0; c0 < R; c0 += 64) {
        A x = (c0 + lane < R) ? (A)cell(c0 + lane) : (A)0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            A y = shfl_up_acc(x, d);
            if (lane >= d) x += y;
        }
        const A pre = carry + x;
        of |= __any(pre < lo || pre > hi) != 0;
        carry = shfl_acc(pre, 63);
    }
    (void)sizeof(T);
    return carry;
}

// ... of row[0..R)
template <int EB>
__device__ __forceinline__ typename Acc<EB>::T checked_row_sum(const typename Elem<EB>::T* row, uint32_t R, int lane, bool& of) {
    return checked_sum_of<EB>([row](uint32_t c) { return row[c]; }, R, lane, of);
}

// at / count / of_code serve the reads by key name (query.hip): answer q goes to slot at[q] (NULL: q), only the
// first *count keys of the list are answered (NULL: all n; the list was appended to by the launch before, so its
// length never visits the host), and an overflow is reported as of_code (jg_pnc_values: 1).
template <int EB>
__global__ __launch_bounds__(kBlock) void k_values(const typename Elem<EB>::T* __restrict__ P, const typename Elem<EB>::T* __restrict__ N,
                                                   uint32_t R, const uint32_t* __restrict__ keys, uint64_t n,
                                                   long long* __restrict__ out, uint8_t* __restrict__ ovf,
                                                   const uint32_t* __restrict__ at, const unsigned long long* __restrict__ count,
                                                   uint8_t of_code) {
    using T = typename Elem<EB>::T;
    using UT = std::make_unsigned_t<T>;
    const int lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * kBlock) >> 6;
    if (count && *count < n) n = *count;
    for (uint64_t q = wave; q < n; q += n_waves) {
        const uint64_t k = keys ? keys[q] : q;
        bool of = false;
        const auto sp = checked_row_sum<EB>(P + k * R, R, lane, of);
        const auto sn = checked_row_sum<EB>(N + k * R, R, lane, of);
        if (lane == 0) {
            // ΣP and ΣN are in range when !of; '-' is unchecked: wrap at the width.
            const T v = (T)((UT)(T)sp - (UT)(T)sn);
            const uint64_t o = at ? at[q] : q;
            out[o] = of ? 0 : (long long)v;
            ovf[o] = of ? of_code : 0;
        }
    }
}

// PNCounter.Get in the middle of a batch (jg_node_exec_keys, update.hip): one wave per read, k_values'
// checked sums over the row with the cell at column `col` replaced by cell + the amounts the batch's earlier commands
// added to it, wrapping at the width as Increment / Decrement do.  Read q is command at[q] on row keys[q]; dp / dn hold,
// by command index, MINUS the amounts on P / N of the row's commands up to and including that command
// (pnc_encode.hip k_prefix_scatter's rewinds; a read adds 0).  It runs in front of k_add_list, so the rows are those
// from before the call.  keys / count / of_code as for k_values; at is required.
template <int EB>
__global__ __launch_bounds__(kBlock) void k_values_at(const typename Elem<EB>::T* __restrict__ P, const typename Elem<EB>::T* __restrict__ N,
                                                      uint32_t R, uint32_t col, const uint32_t* __restrict__ keys, uint64_t n,
                                                      const long long* __restrict__ dp, const long long* __restrict__ dn,
                                                      long long* __restrict__ out, uint8_t* __restrict__ ovf,
                                                      const uint32_t* __restrict__ at, const unsigned long long* __restrict__ count,
                                                      uint8_t of_code) {
    using T = typename Elem<EB>::T;
    using UT = std::make_unsigned_t<T>;
    const int lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * kBlock) >> 6;
    if (count && *count < n) n = *count;
    for (uint64_t q = wave; q < n; q += n_waves) {
        const uint64_t k = keys[q], o = at[q];
        const T *rp = P + k * R, *rn = N + k * R;
        const UT ap = (UT)(0ull - (unsigned long long)dp[o]), an = (UT)(0ull - (unsigned long long)dn[o]);
        bool of = false;
        const auto sp = checked_sum_of<EB>([=](uint32_t c) { return c == col ? (T)((UT)rp[c] + ap) : rp[c]; }, R, lane, of);
        const auto sn = checked_sum_of<EB>([=](uint32_t c) { return c == col ? (T)((UT)rn[c] + an) : rn[c]; }, R, lane, of);
        if (lane == 0) {
            const T v = (T)((UT)(T)sp - (UT)(T)sn);
            out[o] = of ? 0 : (long long)v;
            ovf[o] = of ? of_code : 0;
        }
    }
}

// Re-stride copy (jg_pnc_reserve): the destination is n_units units (16-B vectors where both row sizes are whole
// vectors, else cells) in rows of `dw`; unit (row, col) takes the source's (row, col) where row < src_rows and
// col < sw, zero elsewhere, so every destination unit is written exactly once and no memset runs ahead of the
// copy.  One unit per lane over a flat grid, as k_merge_dense: measured on MI355X on the widen's P array (1M keys,
// 64 -> 128 int64 columns, 1.6 GB moved; tools/tune_reserve.hip) at 0.259 ms = 6.2 TB/s against 0.297 ms for a
// device copy of the old bytes plus a memset of the new ones; 2 / 4 / 8 units in flight per lane 0.265 / 0.289 /
// 0.283 ms, a grid capped at 16 blocks per CU 0.292 ms (4 units per lane: 0.308), plain instead of non-temporal
// accesses the same (0.257);
// past kRestrideBlocks blocks the grid strides.  Stores are coalesced, loads contiguous inside a row.  Index
// arithmetic: the block's first (row, col) comes from one 32-bit divide up front and moves by the grid's step
// (step_rows, step_cols: divided on the host) with a compare; a lane's own unit lies at most kBlock / dw + 1 rows
// further, found by a float reciprocal with a +-1 fix-up (exact: the quotient is at most 257 and dw < 2^30) — no
// 64-bit divide per unit.  Touched once: non-temporal both ways, no LDS.

constexpr uint64_t kRestrideBlocks = 1u << 16;  // x kBlock = 16.8M units a pass (268 MB of vectors)

template <class T>
__global__ __launch_bounds__(kBlock) void k_restride(T* __restrict__ dst, const T* __restrict__ src, uint32_t sw, uint32_t dw, float rdw,
                                                     uint64_t src_rows, uint64_t n_units, uint64_t step_rows, uint32_t step_cols) {
    const uint32_t first = blockIdx.x * kBlock;  // < 2^24 (kRestrideBlocks)
    uint64_t row0 = first / dw;
    uint32_t col0 = first - (uint32_t)row0 * dw;
    for (uint64_t base = first; base < n_units; base += (uint64_t)gridDim.x * kBlock) {
        const uint64_t i = base + threadIdx.x;
        if (i < n_units) {
            const uint32_t c = col0 + threadIdx.x;  // < dw + kBlock
            uint32_t q = (uint32_t)((float)c * rdw);
            uint32_t col = c - q * dw;
            if ((int32_t)col < 0) --q, col += dw;
            else if (col >= dw) ++q, col -= dw;
            const uint64_t row = row0 + q;
            T v{};
            if (row < src_rows && col < sw) v = nt_ld(src + row * sw + col);
            nt_st(dst + i, v);
        }
        row0 += step_rows;
        col0 += step_cols;
        if (col0 >= dw) col0 -= dw, ++row0;
    }
}

void check_keys(const uint32_t* k, uint64_t n, uint64_t n_keys, const char* fn) {
    for (uint64_t i = 0; i < n; ++i)
        JG_REQUIRE(k[i] < n_keys, JG_EINVAL, "%s: key_idx[%llu] = %u out of range (n_keys %llu)", fn,
                   (unsigned long long)i, k[i], (unsigned long long)n_keys);
}

// Upload key indices (validated) to ctx scratch.
uint32_t* upload_keys(jg_ctx* ctx, const uint32_t* key_idx, uint64_t n, uint64_t n_keys, const char* fn) {
    check_keys(key_idx, n, n_keys, fn);
    auto* d = static_cast<uint32_t*>(jg::scratch(ctx, ctx->scratch, n * 4));
    JG_HIP(hipMemcpyAsync(d, key_idx, n * 4, hipMemcpyHostToDevice, ctx->stream));
    return d;
}

// The store's per-key list heads (generation-tagged) and a next[] link per received row (grown to the
// largest batch); gen = this batch's generation.
struct Groups { unsigned long long* head; uint32_t* next; unsigned long long gen; };

void launch_merge_indexed(jg_ctx* ctx, uint32_t eb, void* AP, void* AN, const void* BP, const void* BN, const uint32_t* keys,
                          uint64_t n_rows, uint32_t R, const Groups* g = nullptr) {
    if (g && R >= 32 && ((uint64_t)R * eb) % 16 == 0) {
        JG_REQUIRE(n_rows < kNil, JG_EINVAL, "merge: %llu rows exceed one grouped launch", (unsigned long long)n_rows);
        const unsigned gk = jg::grid_for(ctx, n_rows, kBlock, 16);
        hipLaunchKernelGGL(k_group_link, dim3(gk), dim3(kBlock), 0, ctx->stream, keys, n_rows, g->head, g->next, g->gen);
        constexpr int U = 4;  // rows in flight per wave (U = 8 measured slower, tools/tune_grouped.hip)
        const unsigned grid = jg::grid_for(ctx, (n_rows + U - 1) / U * 64, kBlock, 16);
        jg::dispatch_eb(eb, [&](auto EB) {
            using T = typename Elem<EB()>::T;
            hipLaunchKernelGGL((k_merge_grouped<EB(), U>), dim3(grid), dim3(kBlock), 0, ctx->stream, (T*)AP, (T*)AN, (const T*)BP, (const T*)BN,
                               keys, g->head, g->next, n_rows, R, g->gen);
        });
        JG_HIP(hipGetLastError());
        return;
    }
    if (R >= 32) {
        const unsigned grid = jg::grid_for(ctx, n_rows * 64, kBlock, 16);
        jg::dispatch_eb(eb, [&](auto EB) {
            using T = typename Elem<EB()>::T;
            hipLaunchKernelGGL(k_merge_indexed_rows<EB()>, dim3(grid), dim3(kBlock), 0, ctx->stream, (T*)AP, (T*)AN, (const T*)BP, (const T*)BN,
                               keys, n_rows, R);
        });
        JG_HIP(hipGetLastError());
        return;
    }
    const unsigned grid = jg::grid_for(ctx, n_rows * R, kBlock, 16);
    jg::dispatch_eb(eb, [&](auto EB) {
        using T = typename Elem<EB()>::T;
        hipLaunchKernelGGL(k_merge_indexed<EB()>, dim3(grid), dim3(kBlock), 0, ctx->stream, (T*)AP, (T*)AN, (const T*)BP, (const T*)BN, keys,
                           n_rows, R);
    });
    JG_HIP(hipGetLastError());
}

// The store's group state for a batch of n_rows (allocated on first use; each grouped merge takes the next
// generation, and the heads are cleared once every 2^32 - 1 batches).  nullptr when rows are too narrow
// for the vector path.
const Groups* groups_of(jg_pnc* p, uint64_t n_rows, Groups& g) {
    if (p->R < 32 || ((uint64_t)p->R * p->eb) % 16 != 0) return nullptr;
    if (!p->head.p || p->head_gen == 0xFFFFFFFFull) {
        const bool first = !p->head.p;
        if (first) p->head.alloc(p->n_keys * 8);
        JG_HIP(hipMemsetAsync(p->head.p, 0, p->n_keys * 8, p->ctx->stream));
        p->head_gen = 0;
        // JANUS_TEST_HEAD_GEN: a new store's first generation (tests run batches across the wrap)
        const char* e = first ? std::getenv("JANUS_TEST_HEAD_GEN") : nullptr;
        // clamped below 2^32 - 1: the increment below then gives 1 .. 2^32 - 1, never 0 or 2^32 (a generation
        // whose low 32 bits read 0 would make every head look old)
        if (e) p->head_gen = std::min<unsigned long long>(std::strtoull(e, nullptr, 10), 0xFFFFFFFEull);
    }
    ++p->head_gen;
    if (p->next.bytes < n_rows * 4) {
        JG_HIP(hipStreamSynchronize(p->ctx->stream));  // an earlier launch may still read the old links
        p->next.alloc(n_rows * 4 + n_rows);
    }
    g = Groups{p->head.as<unsigned long long>(), p->next.as<uint32_t>(), p->head_gen};
    return &g;
}

void launch_rows_copy(jg_ctx* ctx, uint32_t eb, void* dst, const void* src, const uint32_t* keys, uint64_t n_rows, uint32_t R,
                      int scatter) {
    const unsigned grid = jg::grid_for(ctx, n_rows * R, kBlock, 16);
    jg::dispatch_eb(eb, [&](auto EB) {
        using T = typename Elem<EB()>::T;
        hipLaunchKernelGGL(k_rows_copy<EB()>, dim3(grid), dim3(kBlock), 0, ctx->stream, (T*)dst, (const T*)src, keys, n_rows, R, scatter);
    });
    JG_HIP(hipGetLastError());
}

template <class T>
void launch_restride_t(jg_ctx* ctx, void* dst, const void* src, uint64_t sw, uint64_t dw, uint64_t src_rows, uint64_t dst_rows) {
    const uint64_t n_units = dst_rows * dw;
    const unsigned grid = (unsigned)std::min<uint64_t>(std::max<uint64_t>((n_units + kBlock - 1) / kBlock, 1), kRestrideBlocks);
    const uint64_t step = (uint64_t)grid * kBlock;
    hipLaunchKernelGGL(k_restride<T>, dim3(grid), dim3(kBlock), 0, ctx->stream, (T*)dst, (const T*)src, (uint32_t)sw, (uint32_t)dw,
                       1.0f / (float)dw, src_rows, n_units, step / dw, (uint32_t)(step % dw));
    JG_HIP(hipGetLastError());
}

// [src_rows x sr] cells of `cell` bytes into [dst_rows x dr] (dr > sr), new cells zero: the vector path where both
// row sizes are whole 16-B vectors (always so for the replica table's Guids), else cell by cell.
void launch_restride(jg_ctx* ctx, uint32_t cell, void* dst, const void* src, uint32_t sr, uint32_t dr, uint64_t src_rows, uint64_t dst_rows) {
    const uint64_t sb = (uint64_t)sr * cell, db = (uint64_t)dr * cell;
    if (sb % 16 == 0 && db % 16 == 0) launch_restride_t<uint4>(ctx, dst, src, sb / 16, db / 16, src_rows, dst_rows);
    else if (cell == 8) launch_restride_t<long long>(ctx, dst, src, sr, dr, src_rows, dst_rows);
    else launch_restride_t<int>(ctx, dst, src, sr, dr, src_rows, dst_rows);
}

// The same rows under more keys (the stride stays): a device copy and the tail zeroed.
void grow_rows(jg_ctx* ctx, void* dst, const void* src, size_t old_bytes, size_t new_bytes) {
    if (old_bytes) JG_HIP(hipMemcpyAsync(dst, src, old_bytes, hipMemcpyDeviceToDevice, ctx->stream));
    if (new_bytes > old_bytes) JG_HIP(hipMemsetAsync((char*)dst + old_bytes, 0, new_bytes - old_bytes, ctx->stream));
}

void swap_buf(jg::DevBuf& a, jg::DevBuf& b) {
    std::swap(a.p, b.p);
    std::swap(a.bytes, b.bytes);
    std::swap(a.own, b.own);
}

}  // namespace

void jg::pnc_merge_indexed(jg_pnc* p, const void* BP, const void* BN, const uint32_t* d_keys, uint64_t n_rows) {
    Groups g;
    launch_merge_indexed(p->ctx, p->eb, p->rw_P(), p->rw_N(), BP, BN, d_keys, n_rows, p->R, groups_of(p, n_rows, g));
}

// The store grown in place to [n_keys x n_replicas] (never shrunk).  Every new buffer is allocated before anything
// is copied and the store's own fields change only after both streams have drained, so a failure at any point
// leaves the store as it was (the new buffers are freed on the way out).  Takes no heed of an open wave: the
// public entry point refuses those, the automatic widening runs inside one (pnc_auto_widen).
void jg::pnc_grow(jg_pnc* p, uint64_t n_keys, uint32_t n_replicas) {
    const uint64_t ok = p->n_keys, nk = std::max(n_keys, ok);
    const uint32_t orr = p->R, nr = std::max(n_replicas, orr), eb = p->eb;
    if (nk == ok && nr == orr) return;
    JG_REQUIRE(nk <= 0xFFFFFFFFull, JG_EINVAL, "jg_pnc_reserve: key_idx is 32-bit (%llu keys)", (unsigned long long)nk);
    JG_REQUIRE(nr < 0x40000000u, JG_EINVAL, "jg_pnc_reserve: at most 2^30-1 replica columns");  // k_restride's index arithmetic
    JG_REQUIRE(!p->cols.p || nr <= jg::kMaxTableReplicas, JG_EINVAL, "jg_pnc_reserve: the replica table holds at most %u replicas per key (%u asked)",
               jg::kMaxTableReplicas, nr);
    JG_REQUIRE(nk * nr <= (1ull << 44), JG_ENOMEM, "jg_pnc_reserve: %llu x %u cells exceed any device", (unsigned long long)nk, nr);
    jg_ctx* ctx = p->ctx;
    jg::ensure_device(ctx);
    const bool table = p->cols.p != nullptr;
    static const bool trace = std::getenv("JANUS_TRACE_RESERVE") != nullptr;  // the call's phases to stderr
    const double t0 = jg::now_us();
    jg::DevBuf nP, nN, nC, nNc;  // all of them first: an allocation failure leaves the store untouched
    nP.alloc((size_t)nk * nr * eb);
    nN.alloc((size_t)nk * nr * eb);
    if (table) {
        nC.alloc((size_t)nk * nr * 16);
        nNc.alloc((size_t)nk * 4);
    }
    if (nr == orr) {
        grow_rows(ctx, nP.p, p->ro_P(), (size_t)ok * orr * eb, nP.bytes);
        grow_rows(ctx, nN.p, p->ro_N(), (size_t)ok * orr * eb, nN.bytes);
        if (table) grow_rows(ctx, nC.p, p->cols.p, (size_t)ok * orr * 16, nC.bytes);
    } else {
        launch_restride(ctx, eb, nP.p, p->ro_P(), orr, nr, ok, nk);
        launch_restride(ctx, eb, nN.p, p->ro_N(), orr, nr, ok, nk);
        if (table) launch_restride(ctx, 16, nC.p, p->cols.p, orr, nr, ok, nk);  // new slots all-zero (json_wave.hpp row_cache)
    }
    if (table) grow_rows(ctx, nNc.p, p->ncols.p, (size_t)ok * 4, nNc.bytes);
    const double t1 = jg::now_us();
    // the old buffers go: everything queued on them first (an async merge_batch on `stream`, the upload stream)
    JG_HIP(hipStreamSynchronize(ctx->stream));
    JG_HIP(hipStreamSynchronize(ctx->copy));
    const double t2 = jg::now_us();
    swap_buf(p->P_, nP);
    swap_buf(p->N_, nN);
    if (table) swap_buf(p->cols, nC), swap_buf(p->ncols, nNc);
    if (nk != ok) p->head.release();  // the grouped merge's heads follow n_keys: first use recreates them (groups_of)
    p->shadow.drop();  // the dense merge's shadow follows the shape (both streams have drained: nothing reads it)
    p->n_keys = nk;
    p->R = nr;
    if (trace) {
        nP.release(), nN.release(), nC.release(), nNc.release();  // the old buffers (freed here or on the way out)
        std::fprintf(stderr, "reserve %llu x %u -> %llu x %u: allocate + queue %.3f ms, copies %.3f ms, free %.3f ms\n", (unsigned long long)ok, orr,
                     (unsigned long long)nk, nr, (t1 - t0) * 1e-3, (t2 - t1) * 1e-3, (jg::now_us() - t2) * 1e-3);
    }
}

// One step of the opt-in widening after a call failed for row capacity (its roll-back has run): R doubles, up to
// the caller's bound and the replica table's.  false = at the bound (or no room on the device): the call's own
// failure stands.
bool jg::pnc_auto_widen(jg_pnc* p) {
    uint64_t cap = p->max_R;
    if (p->cols.p) cap = std::min<uint64_t>(cap, jg::kMaxTableReplicas);
    const uint64_t nr = std::min<uint64_t>(2ull * p->R, cap);
    if (nr <= p->R) return false;
    try {
        pnc_grow(p, p->n_keys, (uint32_t)nr);
    } catch (const jg::Error&) {
        return false;
    }
    return true;
}

extern "C" {

int jg_pnc_create(jg_ctx* ctx, uint64_t n_keys, uint32_t n_replicas, uint32_t elem_bytes, jg_pnc** out) {
    return jg::guard([&] {
        auto lk_ = jg::lock(ctx);  // calls on one context are serialised (shared scratch, stream)
        JG_REQUIRE(ctx && out, JG_EINVAL, "jg_pnc_create: NULL argument");
        JG_REQUIRE(elem_bytes == 4 || elem_bytes == 8, JG_EINVAL, "jg_pnc_create: elem_bytes must be 4 or 8");
        JG_REQUIRE(n_replicas > 0 && n_keys > 0, JG_EINVAL, "jg_pnc_create: empty shape");
        JG_REQUIRE(n_keys <= 0xFFFFFFFFull, JG_EINVAL, "jg_pnc_create: key_idx is 32-bit");
        jg::ensure_device(ctx);
        auto* p = new jg_pnc();
        p->ctx = ctx; p->n_keys = n_keys; p->R = n_replicas; p->eb = elem_bytes;
        try {
            const size_t bytes = (size_t)n_keys * n_replicas * elem_bytes;
            p->P_.alloc(bytes);
            p->N_.alloc(bytes);
            JG_HIP(hipMemsetAsync(p->rw_P(), 0, bytes, ctx->stream));  // PNCounter(): every replica absent = 0
            JG_HIP(hipMemsetAsync(p->rw_N(), 0, bytes, ctx->stream));
            JG_HIP(hipStreamSynchronize(ctx->stream));
        } catch (...) {
            delete p;
            throw;
        }
        *out = p;
    });
}

int jg_pnc_destroy(jg_pnc* p) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        jg::require_writable(p, "jg_pnc_destroy");
        if (!p) return;
        jg::ensure_device(p->ctx);
        JG_HIP(hipStreamSynchronize(p->ctx->stream));
        delete p;
    });
}

int jg_pnc_shape(jg_pnc* p, uint64_t* n_keys, uint32_t* n_replicas, uint32_t* elem_bytes) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        check_store(p, "jg_pnc_shape");
        if (n_keys) *n_keys = p->n_keys;
        if (n_replicas) *n_replicas = p->R;
        if (elem_bytes) *elem_bytes = p->eb;
    });
}

int jg_pnc_reserve(jg_pnc* p, uint64_t n_keys, uint32_t n_replicas) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        jg::require_writable(p, "jg_pnc_reserve");
        check_store(p, "jg_pnc_reserve");
        JG_REQUIRE(!p->wave.is_open(), JG_EINVAL, "jg_pnc_reserve: a wave (jg_pnc_wave_begin) is open on this store");
        jg::pnc_grow(p, n_keys, n_replicas);
    });
}

int jg_pnc_set_max_replicas(jg_pnc* p, uint32_t max_replicas) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        check_store(p, "jg_pnc_set_max_replicas");
        p->max_R = max_replicas;
    });
}

int jg_pnc_write_rows(jg_pnc* p, const uint32_t* key_idx, uint64_t n_rows, const void* P, const void* N) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        jg::require_writable(p, "jg_pnc_write_rows");
        check_store(p, "jg_pnc_write_rows");
        JG_REQUIRE(P && N, JG_EINVAL, "jg_pnc_write_rows: NULL rows");
        if (n_rows == 0) return;
        jg_ctx* ctx = p->ctx;
        jg::ensure_device(ctx);
        const size_t bytes = (size_t)n_rows * p->R * p->eb;
        if (!key_idx) {
            JG_REQUIRE(n_rows <= p->n_keys, JG_EINVAL, "jg_pnc_write_rows: %llu rows > n_keys", (unsigned long long)n_rows);
            JG_HIP(hipMemcpyAsync(p->rw_P(), P, bytes, hipMemcpyHostToDevice, ctx->stream));
            JG_HIP(hipMemcpyAsync(p->rw_N(), N, bytes, hipMemcpyHostToDevice, ctx->stream));
        } else {
            const uint32_t* dk = upload_keys(ctx, key_idx, n_rows, p->n_keys, "jg_pnc_write_rows");
            void* st = jg::scratch(ctx, ctx->scratch2, 2 * bytes);
            JG_HIP(hipMemcpyAsync(st, P, bytes, hipMemcpyHostToDevice, ctx->stream));
            JG_HIP(hipMemcpyAsync((char*)st + bytes, N, bytes, hipMemcpyHostToDevice, ctx->stream));
            launch_rows_copy(ctx, p->eb, p->rw_P(), st, dk, n_rows, p->R, 1);
            launch_rows_copy(ctx, p->eb, p->rw_N(), (char*)st + bytes, dk, n_rows, p->R, 1);
        }
        JG_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int jg_pnc_read_rows(jg_pnc* p, const uint32_t* key_idx, uint64_t n_rows, void* P, void* N) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        check_store(p, "jg_pnc_read_rows");
        JG_REQUIRE(P && N, JG_EINVAL, "jg_pnc_read_rows: NULL rows");
        if (n_rows == 0) return;
        jg_ctx* ctx = p->ctx;
        jg::ensure_device(ctx);
        const size_t bytes = (size_t)n_rows * p->R * p->eb;
        if (!key_idx) {
            JG_REQUIRE(n_rows <= p->n_keys, JG_EINVAL, "jg_pnc_read_rows: %llu rows > n_keys", (unsigned long long)n_rows);
            JG_HIP(hipMemcpyAsync(P, p->ro_P(), bytes, hipMemcpyDeviceToHost, ctx->stream));
            JG_HIP(hipMemcpyAsync(N, p->ro_N(), bytes, hipMemcpyDeviceToHost, ctx->stream));
        } else {
            const uint32_t* dk = upload_keys(ctx, key_idx, n_rows, p->n_keys, "jg_pnc_read_rows");
            void* st = jg::scratch(ctx, ctx->scratch2, 2 * bytes);
            launch_rows_copy(ctx, p->eb, st, p->ro_P(), dk, n_rows, p->R, 0);
            launch_rows_copy(ctx, p->eb, (char*)st + bytes, p->ro_N(), dk, n_rows, p->R, 0);
            JG_HIP(hipMemcpyAsync(P, st, bytes, hipMemcpyDeviceToHost, ctx->stream));
            JG_HIP(hipMemcpyAsync(N, (char*)st + bytes, bytes, hipMemcpyDeviceToHost, ctx->stream));
        }
        JG_HIP(hipStreamSynchronize(ctx->stream));
    });
}

}  // extern "C"

namespace jg {
void pnc_values_device(jg_pnc* p, const uint32_t* d_keys, uint64_t n, long long* d_out, uint8_t* d_ovf, const uint32_t* d_at,
                       const unsigned long long* d_count, uint8_t of_code) {
    jg_ctx* ctx = p->ctx;
    const unsigned grid = jg::grid_for(ctx, n * 64, kBlock, 16);
    dispatch_eb(p->eb, [&](auto EB) {
        using T = typename Elem<EB()>::T;
        hipLaunchKernelGGL(k_values<EB()>, dim3(grid), dim3(kBlock), 0, ctx->stream, (const T*)p->ro_P(), (const T*)p->ro_N(), p->R, d_keys, n, d_out,
                           d_ovf, d_at, d_count, of_code);
    });
    JG_HIP(hipGetLastError());
}

void pnc_values_at_device(jg_pnc* p, uint32_t col, const uint32_t* d_keys, uint64_t n, const long long* d_dp, const long long* d_dn, long long* d_out,
                          uint8_t* d_ovf, const uint32_t* d_at, const unsigned long long* d_count, uint8_t of_code) {
    jg_ctx* ctx = p->ctx;
    JG_REQUIRE(col < p->R, JG_EINVAL, "pnc_values_at_device: column %u outside the store's %u", col, p->R);
    const unsigned grid = jg::grid_for(ctx, n * 64, kBlock, 16);
    dispatch_eb(p->eb, [&](auto EB) {
        using T = typename Elem<EB()>::T;
        hipLaunchKernelGGL(k_values_at<EB()>, dim3(grid), dim3(kBlock), 0, ctx->stream, (const T*)p->ro_P(), (const T*)p->ro_N(), p->R, col, d_keys, n,
                           d_dp, d_dn, d_out, d_ovf, d_at, d_count, of_code);
    });
    JG_HIP(hipGetLastError());
}

void pnc_add_list_device(jg_pnc* p, const uint32_t* d_row, const long long* d_amount, const uint8_t* d_is_n, const unsigned long long* d_count,
                         uint64_t n_max, uint32_t col) {
    jg_ctx* ctx = p->ctx;
    JG_REQUIRE(col < p->R, JG_EINVAL, "pnc_add_list_device: column %u outside the store's %u", col, p->R);
    const unsigned grid = jg::grid_for(ctx, n_max, kBlock, 16);
    dispatch_eb(p->eb, [&](auto EB) {
        using T = typename Elem<EB()>::T;
        hipLaunchKernelGGL(k_add_list<EB()>, dim3(grid), dim3(kBlock), 0, ctx->stream, (T*)p->rw_P(), (T*)p->rw_N(), d_row, d_amount, d_is_n, d_count,
                           n_max, col, p->R);
    });
    JG_HIP(hipGetLastError());
}
}  // namespace jg

extern "C" {

int jg_pnc_merge_rows(jg_pnc* p, const uint32_t* key_idx, uint64_t n_rows, const void* P, const void* N) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        jg::require_writable(p, "jg_pnc_merge_rows");
        check_store(p, "jg_pnc_merge_rows");
        JG_REQUIRE(P && N, JG_EINVAL, "jg_pnc_merge_rows: NULL rows");
        if (n_rows == 0) return;
        jg_ctx* ctx = p->ctx;
        jg::ensure_device(ctx);
        const size_t bytes = (size_t)n_rows * p->R * p->eb;
        const uint32_t* dk = nullptr;
        if (key_idx) dk = upload_keys(ctx, key_idx, n_rows, p->n_keys, "jg_pnc_merge_rows");
        else JG_REQUIRE(n_rows <= p->n_keys, JG_EINVAL, "jg_pnc_merge_rows: %llu rows > n_keys", (unsigned long long)n_rows);
        void* st = jg::scratch(ctx, ctx->scratch2, 2 * bytes);
        JG_HIP(hipMemcpyAsync(st, P, bytes, hipMemcpyHostToDevice, ctx->stream));
        JG_HIP(hipMemcpyAsync((char*)st + bytes, N, bytes, hipMemcpyHostToDevice, ctx->stream));
        Groups g;
        if (dk) launch_merge_indexed(ctx, p->eb, p->rw_P(), p->rw_N(), st, (char*)st + bytes, dk, n_rows, p->R, groups_of(p, n_rows, g));
        else jg::pnc_merge_dense(p, st, (char*)st + bytes, n_rows, false);
        JG_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int jg_pnc_apply_ops(jg_pnc* p, uint64_t n_ops, const uint32_t* key, const uint32_t* col, const int64_t* delta, const uint8_t* is_n) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        jg::require_writable(p, "jg_pnc_apply_ops");
        check_store(p, "jg_pnc_apply_ops");
        if (n_ops == 0) return;
        JG_REQUIRE(key && col && delta && is_n, JG_EINVAL, "jg_pnc_apply_ops: NULL argument");
        for (uint64_t i = 0; i < n_ops; ++i)
            JG_REQUIRE(key[i] < p->n_keys && col[i] < p->R, JG_EINVAL, "jg_pnc_apply_ops: op %llu addresses (%u,%u) outside the store",
                       (unsigned long long)i, key[i], col[i]);
        jg_ctx* ctx = p->ctx;
        jg::ensure_device(ctx);
        uint32_t *dkey, *dcol;
        long long* ddel;
        uint8_t* dn;
        jg::Layout L;
        L.add(dkey, n_ops, 16), L.add(dcol, n_ops, 4), L.add(ddel, n_ops, 16), L.add(dn, n_ops, 1);
        L.bind(jg::scratch(ctx, ctx->scratch2, L.bytes() + 64));
        JG_HIP(hipMemcpyAsync(dkey, key, n_ops * 4, hipMemcpyHostToDevice, ctx->stream));
        JG_HIP(hipMemcpyAsync(dcol, col, n_ops * 4, hipMemcpyHostToDevice, ctx->stream));
        JG_HIP(hipMemcpyAsync(ddel, delta, n_ops * 8, hipMemcpyHostToDevice, ctx->stream));
        JG_HIP(hipMemcpyAsync(dn, is_n, n_ops, hipMemcpyHostToDevice, ctx->stream));
        const unsigned grid = jg::grid_for(ctx, n_ops, kBlock, 16);
        jg::dispatch_eb(p->eb, [&](auto EB) {
            using T = typename Elem<EB()>::T;
            hipLaunchKernelGGL(k_apply_ops<EB()>, dim3(grid), dim3(kBlock), 0, ctx->stream, (T*)p->rw_P(), (T*)p->rw_N(), dkey, dcol, ddel, dn, n_ops,
                               p->R);
        });
        JG_HIP(hipGetLastError());
        JG_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int jg_pnc_values(jg_pnc* p, const uint32_t* key_idx, uint64_t n, int64_t* out, uint8_t* overflow) {
    return jg::guard([&] {
        auto lk_ = jg::lock(p);  // calls on one context are serialised (shared scratch, stream)
        check_store(p, "jg_pnc_values");
        JG_REQUIRE(out && overflow, JG_EINVAL, "jg_pnc_values: NULL output");
        if (n == 0) return;
        jg_ctx* ctx = p->ctx;
        jg::ensure_device(ctx);
        const uint32_t* dk = nullptr;
        if (key_idx) dk = upload_keys(ctx, key_idx, n, p->n_keys, "jg_pnc_values");
        else JG_REQUIRE(n <= p->n_keys, JG_EINVAL, "jg_pnc_values: %llu keys > n_keys", (unsigned long long)n);
        char* st = static_cast<char*>(jg::scratch(ctx, ctx->scratch2, n * 9 + 64));
        long long* dout = (long long*)st;
        uint8_t* dovf = (uint8_t*)(st + n * 8);
        jg::pnc_values_device(p, dk, n, dout, dovf, nullptr, nullptr, 1);
        JG_HIP(hipMemcpyAsync(out, dout, n * 8, hipMemcpyDeviceToHost, ctx->stream));
        JG_HIP(hipMemcpyAsync(overflow, dovf, n, hipMemcpyDeviceToHost, ctx->stream));
        JG_HIP(hipStreamSynchronize(ctx->stream));
    });
}

}  // extern "C"
