// block_scan.hpp — the one block-wide scan of the key-space set's kernels, and the exclusive scan of a long array of
// counts built on it.  Device-only.  block_scan_incl is a template, so tpset_scan.hpp's kernels use it too; the three
// count-scan kernels below it belong to the unit that defines jgt::excl_scan (tpset.hip), the only one that includes
// this file: a second includer would carry a second copy of every kernel here.
#pragma once

#include "tpset_dict.hpp"

namespace {

using jgt::kBlock;
using jgt::ull;

// Hillis-Steele inclusive scan of one value per lane over a block of N lanes: afterwards sh[t] = op(v[0], .., v[t])
// (op's left argument is the earlier span), every lane is past the last barrier, and the lane's own inclusive value
// is returned.  A lane's exclusive prefix is sh[t - 1], the block's total sh[N - 1].  1 + 2 log2(N) barriers.
template <uint32_t N, class T, class Op> __device__ __forceinline__ T block_scan_incl(T v, T* sh, Op op) {
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < N; d <<= 1) {
        v = t >= d ? op(sh[t - d], sh[t]) : sh[t];
        __syncthreads();
        sh[t] = v;
        __syncthreads();
    }
    return v;
}
struct ScanAdd {
    template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};

// exclusive scan of n counts in one block: out[i] = in[0] + .. + in[i-1], out[n] = the total
template <class T> __global__ __launch_bounds__(1024) void k_excl_scan(const T* __restrict__ in, ull* __restrict__ out, uint64_t n) {
    __shared__ ull sh[1024];
    const uint32_t t = threadIdx.x;
    const uint64_t per = (n + 1023) / 1024;
    const uint64_t b = jgt::umin(n, t * per), e = jgt::umin(n, b + per);
    ull sum = 0;
    for (uint64_t i = b; i < e; ++i) sum += in[i];
    block_scan_incl<1024>(sum, sh, ScanAdd{});
    ull run = t ? sh[t - 1] : 0;
    for (uint64_t i = b; i < e; ++i) {
        out[i] = run;
        run += in[i];
    }
    if (t == 1023) out[n] = sh[1023];
}

// The same over many blocks, for the long arrays (one per candidate): per-block sums, the one-block scan over
// them, then each block scans its own tile from its base.  Three launches; no block waits on another.
constexpr uint32_t kScanItems = 8, kScanTile = kBlock * kScanItems;
__device__ __forceinline__ ull scan_tile_load(const uint32_t* __restrict__ in, uint64_t n, uint32_t (&v)[kScanItems]) {
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + threadIdx.x * kScanItems;
    ull s = 0;
#pragma unroll
    for (uint32_t j = 0; j < kScanItems; ++j) {
        v[j] = base + j < n ? in[base + j] : 0;
        s += v[j];
    }
    return s;
}
__global__ __launch_bounds__(kBlock) void k_scan_sum(const uint32_t* __restrict__ in, uint64_t n, ull* __restrict__ bsum) {
    __shared__ ull sh[kBlock];
    uint32_t v[kScanItems];
    sh[threadIdx.x] = scan_tile_load(in, n, v);
    __syncthreads();
    for (uint32_t d = kBlock / 2; d; d >>= 1) {
        if (threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) bsum[blockIdx.x] = sh[0];
}
__global__ __launch_bounds__(kBlock) void k_scan_apply(const uint32_t* __restrict__ in, uint64_t n, const ull* __restrict__ bbase, ull* __restrict__ out) {
    __shared__ ull sh[kBlock];
    const uint32_t t = threadIdx.x;
    uint32_t v[kScanItems];
    block_scan_incl<kBlock>(scan_tile_load(in, n, v), sh, ScanAdd{});
    ull run = bbase[blockIdx.x] + (t ? sh[t - 1] : 0);
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + t * kScanItems;
#pragma unroll
    for (uint32_t j = 0; j < kScanItems; ++j) {
        if (base + j < n) out[base + j] = run;
        run += v[j];
    }
    if (blockIdx.x == 0 && t == 0) out[n] = bbase[gridDim.x];
}

}  // namespace
