// tools/tune_reserve.hip — jg_pnc_reserve beside its yardstick, in one run (make tools; build/tune_reserve).
//
// Two shapes at 1M keys, int64, the replica table present:
//   widen    64 -> 128 columns (the re-stride kernel k_restride over P, N and the table)
//   keys     1M -> 2M keys at 64 columns (device copies and tail memsets)
// The yardstick moves the same bytes the plain way: hipMemcpyAsync device-to-device of the old bytes and
// hipMemsetAsync of the added bytes, into buffers of the same sizes (allocated outside the timed part, as the
// yardstick of a copy should be; the reserve's own allocations and frees are inside its time, and the library prints
// them phase by phase under JANUS_TRACE_RESERVE, which this tool sets).  1 warm-up and the median of 5, each repetition
// on a newly created store.  Bytes per second = (old bytes read + new bytes written) / time; the bar is reserve >=
// 0.8 x yardstick.  Last: the re-stride kernel's variants on one array beside the same yardstick, device-timed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "janus_gpu.h"

#define HIP_OK(x)                                                                        \
    do {                                                                                 \
        hipError_t e_ = (x);                                                             \
        if (e_ != hipSuccess) {                                                          \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                 \
            std::exit(2);                                                                \
        }                                                                                \
    } while (0)

static void jg_ok(int rc, const char* what) {
    if (rc == JG_OK) return;
    char buf[512];
    jg_last_error(buf, sizeof buf);
    std::fprintf(stderr, "%s: [%d] %s\n", what, rc, buf);
    std::exit(2);
}

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static double median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

// ---- the re-stride kernel's variants on one array (P of the widen: 1M x 64 -> 128 int64), device-timed -------------
// csrc/pnc.hip's k_restride restated with its two choices open: NT = non-temporal loads and stores, U = units a lane
// has in flight (a block owns U x 256 consecutive destination vectors), and the grid flat or capped at `cap` blocks.
typedef unsigned int v4u __attribute__((ext_vector_type(4)));
template <bool NT, int U>
__global__ __launch_bounds__(256) void k_variant(v4u* __restrict__ dst, const v4u* __restrict__ src, uint32_t sw, uint32_t dw, float rdw,
                                                 uint64_t src_rows, uint64_t n_units, uint64_t step_rows, uint32_t step_cols) {
    constexpr uint32_t kTile = 256 * U;
    const uint32_t first = blockIdx.x * kTile;
    uint64_t row0 = first / dw;
    uint32_t col0 = first - (uint32_t)row0 * dw;
    for (uint64_t base = first; base < n_units; base += (uint64_t)gridDim.x * kTile) {
        v4u v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t i = base + u * 256 + threadIdx.x;
            const uint32_t c = col0 + u * 256 + threadIdx.x;
            uint32_t q = (uint32_t)((float)c * rdw);
            uint32_t col = c - q * dw;
            if ((int32_t)col < 0) --q, col += dw;
            else if (col >= dw) ++q, col -= dw;
            const uint64_t row = row0 + q;
            v[u] = v4u{0, 0, 0, 0};
            if (i < n_units && row < src_rows && col < sw) v[u] = NT ? __builtin_nontemporal_load(src + row * sw + col) : src[row * sw + col];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t i = base + u * 256 + threadIdx.x;
            if (i < n_units) {
                if (NT) __builtin_nontemporal_store(v[u], dst + i);
                else dst[i] = v[u];
            }
        }
        row0 += step_rows;
        col0 += step_cols;
        if (col0 >= dw) col0 -= dw, ++row0;
    }
}

template <bool NT, int U>
static double time_variant(hipStream_t st, void* dst, const void* src, uint64_t rows, uint32_t sw, uint32_t dw, uint64_t cap) {
    const uint64_t n_units = rows * dw;
    uint64_t grid = (n_units + 256 * U - 1) / (256 * U);
    if (cap && grid > cap) grid = cap;
    const uint64_t step = grid * 256 * U;
    hipEvent_t a, b;
    HIP_OK(hipEventCreate(&a));
    HIP_OK(hipEventCreate(&b));
    std::vector<double> t;
    for (int rep = 0; rep <= 5; ++rep) {
        HIP_OK(hipEventRecord(a, st));
        hipLaunchKernelGGL((k_variant<NT, U>), dim3((unsigned)grid), dim3(256), 0, st, (v4u*)dst, (const v4u*)src, sw, dw, 1.0f / (float)dw, rows,
                           n_units, step / dw, (uint32_t)(step % dw));
        HIP_OK(hipEventRecord(b, st));
        HIP_OK(hipEventSynchronize(b));
        float ms = 0;
        HIP_OK(hipEventElapsedTime(&ms, a, b));
        if (rep) t.push_back(ms);
    }
    HIP_OK(hipEventDestroy(a));
    HIP_OK(hipEventDestroy(b));
    return median(t);
}

static void variants(hipStream_t st) {
    const uint64_t rows = 1u << 20;
    const uint32_t sw = 64 * 8 / 16, dw = 128 * 8 / 16;
    const size_t ob = rows * sw * 16, nb = rows * dw * 16;
    void *src, *dst;
    HIP_OK(hipMalloc(&src, ob));
    HIP_OK(hipMalloc(&dst, nb));
    HIP_OK(hipMemsetAsync(src, 1, ob, st));
    HIP_OK(hipStreamSynchronize(st));
    hipEvent_t a, b;
    HIP_OK(hipEventCreate(&a));
    HIP_OK(hipEventCreate(&b));
    std::vector<double> t;
    for (int rep = 0; rep <= 5; ++rep) {
        HIP_OK(hipEventRecord(a, st));
        HIP_OK(hipMemcpyAsync(dst, src, ob, hipMemcpyDeviceToDevice, st));
        HIP_OK(hipMemsetAsync(static_cast<char*>(dst) + ob, 0, nb - ob, st));
        HIP_OK(hipEventRecord(b, st));
        HIP_OK(hipEventSynchronize(b));
        float ms = 0;
        HIP_OK(hipEventElapsedTime(&ms, a, b));
        if (rep) t.push_back(ms);
    }
    const double gb = (double)(ob + nb) / 1e9;
    const double ty = median(t);
    std::printf("{\"variant\": \"copy+memset\", \"ms\": %.3f, \"GBps\": %.0f}\n", ty, gb / ty * 1e3);
#define VARIANT(NT, U, CAP)                                                                                        \
    {                                                                                                              \
        const double ms = time_variant<NT, U>(st, dst, src, rows, sw, dw, CAP);                                    \
        std::printf("{\"variant\": \"nt=%d U=%d cap=%d\", \"ms\": %.3f, \"GBps\": %.0f, \"ratio\": %.3f}\n", NT, U, CAP, ms, gb / ms * 1e3, ty / ms); \
    }
    VARIANT(true, 1, 0) VARIANT(false, 1, 0) VARIANT(true, 2, 0) VARIANT(true, 4, 0) VARIANT(false, 4, 0) VARIANT(true, 8, 0)
    VARIANT(true, 1, 4096) VARIANT(true, 4, 4096) VARIANT(false, 4, 4096) VARIANT(true, 4, 2048) VARIANT(true, 1, 65536)
#undef VARIANT
    std::fflush(stdout);
    HIP_OK(hipEventDestroy(a));
    HIP_OK(hipEventDestroy(b));
    HIP_OK(hipFree(src));
    HIP_OK(hipFree(dst));
}

struct Shape { const char* name; uint64_t k0; uint32_t r0; uint64_t k1; uint32_t r1; };

int main() {
    constexpr uint32_t kEb = 8;
    constexpr int kReps = 5;
    setenv("JANUS_TRACE_RESERVE", "1", 0);  // each reserve's phases (allocate, copies, free) to stderr
    jg_ctx* ctx = nullptr;
    jg_ok(jg_open(0, &ctx), "jg_open");
    void* stream_v = nullptr;
    jg_ok(jg_stream(ctx, &stream_v), "jg_stream");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const Shape shapes[2] = {{"widen_64_to_128_cols_1M_keys", 1u << 20, 64, 1u << 20, 128}, {"keys_1M_to_2M_64_cols", 1u << 20, 64, 2u << 20, 64}};
    for (const Shape& s : shapes) {
        // P, N, the Guid table, the column counts
        const size_t old_b[4] = {(size_t)s.k0 * s.r0 * kEb, (size_t)s.k0 * s.r0 * kEb, (size_t)s.k0 * s.r0 * 16, (size_t)s.k0 * 4};
        const size_t new_b[4] = {(size_t)s.k1 * s.r1 * kEb, (size_t)s.k1 * s.r1 * kEb, (size_t)s.k1 * s.r1 * 16, (size_t)s.k1 * 4};
        double moved = 0;
        for (int i = 0; i < 4; ++i) moved += (double)old_b[i] + (double)new_b[i];

        std::vector<double> t_res, t_yard;
        for (int rep = 0; rep <= kReps; ++rep) {  // rep 0 warms up
            jg_pnc* p = nullptr;
            jg_ok(jg_pnc_create(ctx, s.k0, s.r0, kEb, &p), "jg_pnc_create");
            const uint32_t key = 0;
            const jg_guid g{1, 2};
            uint32_t col = 0;
            jg_ok(jg_pnc_intern(p, 1, &key, &g, &col), "jg_pnc_intern");  // the replica table exists
            jg_ok(jg_fence(ctx), "jg_fence");
            const double t0 = now_s();
            jg_ok(jg_pnc_reserve(p, s.k1, s.r1), "jg_pnc_reserve");  // returns with the copies done
            const double t1 = now_s();
            jg_ok(jg_pnc_destroy(p), "jg_pnc_destroy");
            if (rep) t_res.push_back(t1 - t0);
        }
        void *src[4], *dst[4];
        for (int i = 0; i < 4; ++i) {
            HIP_OK(hipMalloc(&src[i], old_b[i]));
            HIP_OK(hipMalloc(&dst[i], new_b[i]));
            HIP_OK(hipMemsetAsync(src[i], 1, old_b[i], stream));
        }
        HIP_OK(hipStreamSynchronize(stream));
        for (int rep = 0; rep <= kReps; ++rep) {
            const double t0 = now_s();
            for (int i = 0; i < 4; ++i) {
                HIP_OK(hipMemcpyAsync(dst[i], src[i], old_b[i], hipMemcpyDeviceToDevice, stream));
                HIP_OK(hipMemsetAsync(static_cast<char*>(dst[i]) + old_b[i], 0, new_b[i] - old_b[i], stream));
            }
            HIP_OK(hipStreamSynchronize(stream));
            const double t1 = now_s();
            if (rep) t_yard.push_back(t1 - t0);
        }
        for (int i = 0; i < 4; ++i) {
            HIP_OK(hipFree(src[i]));
            HIP_OK(hipFree(dst[i]));
        }
        const double tr = median(t_res), ty = median(t_yard);
        std::printf("{\"shape\": \"%s\", \"bytes_moved\": %.0f, \"reserve_ms\": %.3f, \"reserve_GBps\": %.1f, \"yardstick_ms\": %.3f, "
                    "\"yardstick_GBps\": %.1f, \"ratio\": %.3f, \"bar\": 0.8}\n",
                    s.name, moved, tr * 1e3, moved / tr / 1e9, ty * 1e3, moved / ty / 1e9, ty / tr);
        std::fflush(stdout);
    }
    variants(stream);
    jg_ok(jg_close(ctx), "jg_close");
    return 0;
}
