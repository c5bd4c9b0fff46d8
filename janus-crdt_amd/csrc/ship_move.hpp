// ship_move.hpp — the mover of jg_node_update_keys_ship (update.hip): a segmented byte copy on the device.
// A header of its own so that tools/tune_ship_move.hip times the very kernel the library launches.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {  // internal to each file that includes this, like the kernels that use it

// The mover: the shipping commands' bytes from where their encoders wrote them (the PN-Counter list, one region per
// OR-Set round) to their place in the merged image, a segmented byte copy.  Command i's bytes are src[i] .. + (off[i+1] -
// off[i]) (an absolute device address; not read for an empty command) and go to image + off[i].  A workgroup owns kMoveCmds
// consecutive commands, i.e. one contiguous span of the image, and walks the span's aligned 16-byte chunks: a chunk
// inside one command is two aligned 16-byte loads of its source funnel-shifted by the source's misalignment and one
// aligned 16-byte store; a chunk that holds a command boundary (one per command at most) or one of the span's two ends
// is gathered byte by byte.  The aligned loads read up to 15 bytes in front of and 31 bytes behind a command's bytes:
// every source buffer starts 16-byte aligned and is allocated 64 bytes past its bytes.  Nothing is shared between
// workgroups and nothing is published inside the launch.
constexpr int kMoveCmds = 32, kMoveBlock = 256;

__device__ __forceinline__ uint4 shift_bytes(const uint4 v, const uint4 w, uint32_t sh) {  // bytes [sh, sh + 16) of v | w
    const uint32_t a[8] = {v.x, v.y, v.z, v.w, w.x, w.y, w.z, w.w};
    const uint32_t ws = sh >> 2, bits = (sh & 3) * 8;
    uint32_t r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t lo = ws == 0 ? a[j] : ws == 1 ? a[j + 1] : ws == 2 ? a[j + 2] : a[j + 3];
        const uint32_t hi = ws == 0 ? a[j + 1] : ws == 1 ? a[j + 2] : ws == 2 ? a[j + 3] : a[j + 4];
        r[j] = (uint32_t)((((unsigned long long)hi << 32) | lo) >> bits);
    }
    return uint4{r[0], r[1], r[2], r[3]};
}

__global__ __launch_bounds__(kMoveBlock) void k_ship_move(const unsigned long long* __restrict__ src, const unsigned long long* __restrict__ off,
                                                           uint64_t n, uint8_t* __restrict__ image) {
    using ull = unsigned long long;
    __shared__ ull s_off[kMoveCmds + 1], s_src[kMoveCmds];
    const uint64_t first = (uint64_t)blockIdx.x * kMoveCmds;
    const uint32_t m = (uint32_t)(first + kMoveCmds < n ? kMoveCmds : n - first);
    if (threadIdx.x <= m) s_off[threadIdx.x] = off[first + threadIdx.x];
    if (threadIdx.x < m) s_src[threadIdx.x] = src[first + threadIdx.x];
    __syncthreads();
    const ull lo = s_off[0], hi = s_off[m];
    if (hi == lo) return;
    const ull a0 = lo & ~15ull, chunks = (hi - a0 + 15) >> 4;  // image is 16-byte aligned
    for (ull k = threadIdx.x; k < chunks; k += kMoveBlock) {
        const ull b0 = a0 + 16 * k, b1 = b0 + 16;
        const ull p0 = b0 > lo ? b0 : lo, p1 = b1 < hi ? b1 : hi;
        uint32_t c = 0, r = m;  // the command holding byte p0: the last one that begins at or before it
        while (r - c > 1) {
            const uint32_t mid = (c + r) >> 1;
            if (s_off[mid] <= p0) c = mid;
            else r = mid;
        }
        if (p0 == b0 && p1 == b1 && s_off[c + 1] >= b1) {
            const ull S = s_src[c] + (b0 - s_off[c]);
            const uint32_t sh = (uint32_t)(S & 15);
            const uint4* q = reinterpret_cast<const uint4*>(S - sh);
            uint4 v = q[0];
            if (sh) v = shift_bytes(v, q[1], sh);
            *reinterpret_cast<uint4*>(image + b0) = v;
        } else {
            for (ull p = p0; p < p1; ++p) {
                while (s_off[c + 1] <= p) ++c;  // p < hi = s_off[m]
                image[p] = *reinterpret_cast<const uint8_t*>(s_src[c] + (p - s_off[c]));
            }
        }
    }
}

// n > 0 commands, queued on `stream`; the caller checks hipGetLastError
inline void ship_move(hipStream_t stream, const unsigned long long* src, const unsigned long long* off, uint64_t n, uint8_t* image) {
    hipLaunchKernelGGL(k_ship_move, dim3((unsigned)((n + kMoveCmds - 1) / kMoveCmds)), dim3(kMoveBlock), 0, stream, src, off, n, image);
}

}  // namespace
