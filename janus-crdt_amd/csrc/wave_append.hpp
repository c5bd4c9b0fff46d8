// wave_append.hpp — a wave's lanes appended to a device list with one ballot and one atomic per wave, shared by the
// reads and the writes by key name (query.hip, update.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace jg {

// slot of this lane in a list the wave appends `take` lanes to: one atomic per wave.  Every lane of the wave calls it
// (the ballot and the shuffle are wave-wide); the order of the waves in the list is whatever their atomics gave.
__device__ __forceinline__ unsigned long long wave_append(bool take, unsigned long long* count) {
    using ull = unsigned long long;
    const ull mask = __ballot(take);
    if (mask == 0) return 0;
    const int lane = threadIdx.x & 63, first = __ffsll(mask) - 1;
    ull base = 0;
    if (lane == first) base = atomicAdd(count, (ull)__popcll(mask));
    base = __shfl(base, first, 64);
    return base + __popcll(mask & ((1ull << lane) - 1));
}

}  // namespace jg
