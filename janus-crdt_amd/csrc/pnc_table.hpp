// pnc_table.hpp — what json.hip and pnc_encode.hip both need of a PN-Counter store's replica table and of the row-key
// sort: shared by header (as tpset_dict.hpp is), so each file holds its own copy of the kernel and of the sort's.
//
// Replica table (jg_pnc::cols / ncols, allocated on first use): [n_keys x R] Guids + [n_keys] counts.
// P and N share one column per replica: the reference keeps two dictionaries whose key orders coincide
// for every state its nodes produce (constructor inserts self into both, Merge inserts new keys in
// message order), which the shared order reproduces.
#pragma once

#include <hipcub/hipcub.hpp>

#include "launch.hpp"
#include "pnc_wire.hpp"

namespace {  // internal to each file that includes this, like the kernels that use it

inline void ensure_table(jg_pnc* p) {
    if (p->cols.p) return;
    JG_REQUIRE(p->R <= kMaxJsonReplicas, JG_EINVAL, "replica table: at most %u replicas per key (store has %u)", kMaxJsonReplicas, p->R);
    p->cols.alloc((size_t)p->n_keys * p->R * sizeof(Guid16));
    p->ncols.alloc((size_t)p->n_keys * 4);
    JG_HIP(hipMemsetAsync(p->cols.p, 0, p->cols.bytes, p->ctx->stream));  // unused slots are zero (json_wave.hpp row_cache)
    JG_HIP(hipMemsetAsync(p->ncols.p, 0, p->ncols.bytes, p->ctx->stream));
}

inline Table table_of(jg_pnc* p) { return Table{p->cols.as<Guid16>(), p->ncols.as<uint32_t>(), p->R}; }

// keys[j] = row << 32 | i of entry i = j, or (REV) of entry i = n - 1 - j: the entries in order, or newest first.
template <bool REV>
__global__ void k_make_keys(const uint32_t* __restrict__ rows, uint64_t n, unsigned long long* __restrict__ keys) {
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j < n) {
        const uint64_t i = REV ? n - 1 - j : j;
        keys[j] = (unsigned long long)rows[i] << 32 | i;
    }
}

// Radix sorts of the (row << 32 | index) keys on the row bits: Onesweep at every size.  hipcub's default takes a
// block sort plus merge passes below 1M items (the config's merge_sort_limit), ~200 us for a C5 wave's ~0.5M
// deferred entries, whatever the bit range; three 8-bit Onesweep passes cover 1M rows.
using OnesweepSort = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, rocprim::default_config, 0>;
inline hipError_t sort_row_keys(void* tmp, size_t& bytes, const unsigned long long* in, unsigned long long* out, uint64_t n, int end_bit,
                                hipStream_t stream) {
    return rocprim::radix_sort_keys<OnesweepSort>(tmp, bytes, in, out, (size_t)n, 32u, (unsigned)end_bit, stream);
}

// The sort's end bit: the index bits and the row bits of a store of n_keys rows.
inline int row_end_bit(uint64_t n_keys) {
    int row_bits = 1;
    while (row_bits < 32 && (1ull << row_bits) < n_keys) ++row_bits;
    return 32 + row_bits;
}

// Sort `n` 64-bit keys (row << 32 | index) through ctx scratch.  end_bit covers the row bits; the keys arrive in
// index order, forward or reverse (k_make_keys), so a stable sort on the row bits alone keeps that order per row.
inline unsigned long long* sort_keys(jg_ctx* ctx, unsigned long long* keys, uint64_t n, uint64_t n_keys) {
    JG_REQUIRE(n <= 0x7FFFFFFFull, JG_EINVAL, "sort: %llu entries exceed one radix sort", (unsigned long long)n);
    const int end_bit = row_end_bit(n_keys);
    unsigned long long* out = nullptr;
    const auto sort = [&](void* temp, size_t& bytes) { return sort_row_keys(temp, bytes, keys, out, n, end_bit, ctx->stream); };
    const size_t temp = jg::cub_temp_bytes(sort);
    uint8_t* tmp;
    jg::Layout L;
    L.add(out, n), L.add(tmp, temp);
    L.bind(jg::scratch(ctx, ctx->scratch3, L.bytes() + 256));
    jg::cub_run(jg::cub_in(tmp, temp), sort);
    return out;
}

}  // namespace
