// snap_survivors.hpp — who ships a snapshot in a batch of commands resolved on the device: the
// client batcher's rule (SafeCRDTManager.cs:178-181, 186-187) over an object key, whatever the object's kind.  The
// PN-Counter snapshots of jg_node_update_keys_encode key it by row, the OR-Set snapshots of jg_node_update_keys_ship by
// set id; both run these three kernels (pnc_encode.hip launches them, the includer defines kBlock).
//
// The batch is sorted stably on the object key (sorted[s] = key << 32 | command index, seg[s] = the key), with the
// commands that touch no object of the kind under `none_key`, behind every real key.  Sorted position s heads its
// object's run when its key differs from the one before it; an inclusive max-scan of (head ? s : 0) then gives every
// position its run's head.
#pragma once

#include <hipcub/hipcub.hpp>

#include "launch.hpp"

namespace {  // internal to each file that includes this, like the kernels that use it

__global__ void k_snap_heads(const uint32_t* __restrict__ seg, uint64_t n, uint32_t* __restrict__ head) {
    const uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s < n) head[s] = s && seg[s] != seg[s - 1] ? (uint32_t)s : 0u;
}

// the batcher's compaction (SafeCRDTManager.cs:179, 186-187): per run, the latest position with snap == 2, + 1
__global__ void k_snap_latest(const unsigned long long* __restrict__ sorted, uint64_t n, const uint32_t* __restrict__ seg, uint32_t none_key,
                              const uint8_t* __restrict__ snap, const uint32_t* __restrict__ head, uint32_t* __restrict__ latest) {
    const uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n || seg[s] == none_key) return;
    if (snap[(uint32_t)sorted[s]] == 2) atomicMax(&latest[head[s]], (uint32_t)s + 1);
}

// command i ships a snapshot: an applied command on an object of the kind with snap 1, or with snap 2 and no later 2 on
// its object.  none[i] = it does not (the hashes' zero flag), take[i] = it does (the flags positions are scanned from).
__global__ void k_snap_take(const unsigned long long* __restrict__ sorted, uint64_t n, const uint32_t* __restrict__ seg, uint32_t none_key,
                            const uint8_t* __restrict__ snap, const uint32_t* __restrict__ head, const uint32_t* __restrict__ latest,
                            uint8_t* __restrict__ none, uint32_t* __restrict__ take) {
    const uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n) return;
    const uint32_t i = (uint32_t)sorted[s];
    const uint32_t sn = snap ? snap[i] : 1;
    const bool t = seg[s] != none_key && (sn == 1 || (sn == 2 && latest[head[s]] == (uint32_t)s + 1));
    none[i] = !t;
    take[i] = t;
}

// The three launches with the scan between them.  mark, head, latest: n words of the caller's each; tmp: the scan's
// workspace (jg::cub_in); n_i = cub_count(n).
template <class Tmp>
void snap_survivors(jg_ctx* ctx, const unsigned long long* sorted, const uint32_t* seg, uint64_t n, int n_i, uint32_t none_key, const uint8_t* snap,
                    uint32_t* mark, uint32_t* head, uint32_t* latest, uint8_t* none, uint32_t* take, Tmp&& tmp) {
    const unsigned g = jg::blocks_for(n);
    hipLaunchKernelGGL(k_snap_heads, dim3(g), dim3(kBlock), 0, ctx->stream, seg, n, mark);
    JG_HIP(hipGetLastError());
    jg::cub_run(tmp, [&](void* temp, size_t& bytes) { return hipcub::DeviceScan::InclusiveScan(temp, bytes, mark, head, hipcub::Max(), n_i, ctx->stream); });
    if (snap) {
        JG_HIP(hipMemsetAsync(latest, 0, n * 4, ctx->stream));
        hipLaunchKernelGGL(k_snap_latest, dim3(g), dim3(kBlock), 0, ctx->stream, sorted, n, seg, none_key, snap, head, latest);
    }
    hipLaunchKernelGGL(k_snap_take, dim3(g), dim3(kBlock), 0, ctx->stream, sorted, n, seg, none_key, snap, head, latest, none, take);
    JG_HIP(hipGetLastError());
}

}  // namespace
