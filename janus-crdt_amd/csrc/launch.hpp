// launch.hpp — the host-side plumbing every csrc/*.hip shares around its kernels: capped grids, growing device
// buffers, the two-phase hipcub call, the element-width dispatch and the trace clock.  The HIP-free parts (rounding,
// blocks_for, cub_count, Layout) are in layout.hpp.
#pragma once

#include <algorithm>
#include <chrono>
#include <type_traits>
#include <utility>
#include <vector>

#include "jg_internal.hpp"
#include "layout.hpp"

namespace jg {

// Workgroups of `block` threads for a grid-stride kernel over `items`: at least one, at most per_cu on every CU.
inline unsigned grid_for(const jg_ctx* ctx, uint64_t items, unsigned block, unsigned per_cu) {
    const uint64_t g = (items + block - 1) / block, cap = (uint64_t)ctx->num_cus * per_cu;
    return (unsigned)(g > cap ? cap : (g ? g : 1));
}

// At least `bytes` (contents lost when it grows, with a quarter of head room).
inline void ensure(DevBuf& b, size_t bytes) {
    if (b.bytes < bytes) b.alloc(bytes + bytes / 4 + 256);
}

// Grow to `need` bytes keeping the first `keep` bytes; the new tail is zeroed when `zero`.
// retire: the old block goes there instead of hipFree (the element table grows wave after wave, and each
// hipFree costs ~0.2 ms of host time on the box: six arrays per growth); freed by jg::orset_free_retired at the
// end of the wave (node wave, synchronous merge).
inline void grow_keep(jg_ctx* ctx, DevBuf& b, size_t need, size_t keep, bool zero = false, std::vector<void*>* retire = nullptr) {
    if (b.bytes >= need) return;
    if (ctx->copy) JG_HIP(hipStreamSynchronize(ctx->copy));  // uploads still landing in the old block
    DevBuf nb;
    nb.alloc(need + need / 2);
    if (zero) JG_HIP(hipMemsetAsync(nb.p, 0, nb.bytes, ctx->stream));
    keep = std::min(keep, b.p ? b.bytes : 0);
    if (keep) JG_HIP(hipMemcpyAsync(nb.p, b.p, keep, hipMemcpyDeviceToDevice, ctx->stream));
    // a retired block lives until the wave has drained: the kernels queued before this copy may still use it, and
    // those queued after it use the new one (stream order) — no host wait in the middle of a commit (~30 us each,
    // six arrays per names growth).  A block freed right here needs the stream idle first.
    if (!retire) JG_HIP(hipStreamSynchronize(ctx->stream));
    std::swap(nb.p, b.p);
    std::swap(nb.bytes, b.bytes);
    if (retire && nb.p) {
        retire->push_back(nb.p);
        nb.p = nullptr;
        nb.bytes = 0;
    }
}

// A hipcub call is given as `[&](void* temp, size_t& bytes) { return hipcub::X(temp, bytes, ...); }`: asked for its
// temporary size with a null temp, then run on at least that many bytes from `provide(bytes) -> void*`.
template <class Call> size_t cub_temp_bytes(Call&& call) {
    size_t bytes = 0;
    JG_HIP(call(nullptr, bytes));
    return bytes;
}
template <class Provide, class Call> void cub_run(Provide&& provide, Call&& call) {
    size_t bytes = cub_temp_bytes(call);
    void* temp = provide(bytes);
    JG_HIP(call(temp, bytes));
}
// The providers: a buffer of its own grown with ensure, a context scratch buffer, a slice of a carved block.
inline auto cub_in(DevBuf& b) { return [&b](size_t bytes) { return ensure(b, bytes), b.p; }; }
inline auto cub_in(jg_ctx* ctx, DevBuf& b) { return [ctx, &b](size_t bytes) { return scratch(ctx, b, bytes); }; }
inline auto cub_in(void* slice, size_t cap) {
    return [slice, cap](size_t bytes) {
        JG_REQUIRE(bytes <= cap, JG_EINVAL, "hipcub asks for %zu temporary bytes, the block holds %zu", bytes, cap);
        return slice;
    };
}

// f(std::integral_constant<int, 8 | 4>) for a store of 8- or 4-byte counters: `[&](auto EB) { launch<EB()>(...); }`.
template <class F> decltype(auto) dispatch_eb(uint32_t eb, F&& f) {
    if (eb == 8) return f(std::integral_constant<int, 8>{});
    return f(std::integral_constant<int, 4>{});
}

// The clock of the JANUS_TRACE_* lines.
inline double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace jg
