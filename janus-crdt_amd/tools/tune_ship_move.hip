// tools/tune_ship_move.hip — the mover of jg_node_update_keys_ship (csrc/ship_move.hpp) beside
// hipMemcpyAsync device-to-device of the same total bytes, alternating in one process, by hipEvents.
// n commands (default 200,000) with snapshot lengths uniform in [200, 2400) bytes (the ORSetWorkload shape's states), a
// tenth of them empty, their sources spread over two regions with random gaps below 16 bytes, so source and destination
// misalignments are independent.  The result is compared with a host copy once; then 2 warm-ups and the median of 7.
// usage: tune_ship_move [n_commands]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "ship_move.hpp"

#define CHECK(call)                                                                                    \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            std::fprintf(stderr, "%s failed: %s (%s:%d)\n", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            std::exit(1);                                                                              \
        }                                                                                              \
    } while (0)

int main(int argc, char** argv) {
    using ull = unsigned long long;
    const uint64_t n = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 200000;
    std::mt19937_64 rng(15);
    std::vector<ull> len(n), off(n + 1, 0), rel(n);
    std::vector<uint8_t> reg(n);
    ull used[2] = {0, 0};
    for (uint64_t i = 0; i < n; ++i) {
        len[i] = rng() % 10 == 0 ? 0 : 200 + rng() % 2200;
        reg[i] = rng() & 1;
        used[reg[i]] += rng() % 16;
        rel[i] = used[reg[i]];
        used[reg[i]] += len[i];
        off[i + 1] = off[i] + len[i];
    }
    const ull total = off[n];
    std::vector<uint8_t> h[2];
    uint8_t* d[2];
    for (int r = 0; r < 2; ++r) {
        h[r].resize(used[r] + 64);
        for (uint8_t& b : h[r]) b = (uint8_t)rng();
        CHECK(hipMalloc(&d[r], h[r].size()));
        CHECK(hipMemcpy(d[r], h[r].data(), h[r].size(), hipMemcpyHostToDevice));
    }
    std::vector<ull> src(n);
    std::vector<uint8_t> want(total);
    for (uint64_t i = 0; i < n; ++i) {
        src[i] = (ull)(uintptr_t)d[reg[i]] + rel[i];
        if (len[i]) std::memcpy(want.data() + off[i], h[reg[i]].data() + rel[i], len[i]);
    }
    ull *d_src, *d_off;
    uint8_t *image, *plain;
    CHECK(hipMalloc(&d_src, n * 8));
    CHECK(hipMalloc(&d_off, (n + 1) * 8));
    CHECK(hipMalloc(&image, total + 64));
    CHECK(hipMalloc(&plain, total + 64));
    CHECK(hipMemcpy(d_src, src.data(), n * 8, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_off, off.data(), (n + 1) * 8, hipMemcpyHostToDevice));
    CHECK(hipMemset(image, 0xEE, total + 64));
    hipStream_t stream;
    CHECK(hipStreamCreate(&stream));
    ship_move(stream, d_src, d_off, n, image);
    CHECK(hipGetLastError());
    CHECK(hipStreamSynchronize(stream));
    std::vector<uint8_t> got(total + 64);
    CHECK(hipMemcpy(got.data(), image, total + 64, hipMemcpyDeviceToHost));
    if (std::memcmp(got.data(), want.data(), total) != 0 || !std::all_of(got.begin() + total, got.end(), [](uint8_t b) { return b == 0xEE; })) {
        std::fprintf(stderr, "the mover's image differs from the host's copy\n");
        return 2;
    }
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    std::vector<float> tm, tc;
    for (int r = 0; r < 9; ++r) {
        float ms;
        CHECK(hipEventRecord(e0, stream));
        ship_move(stream, d_src, d_off, n, image);
        CHECK(hipEventRecord(e1, stream));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (r >= 2) tm.push_back(ms);
        CHECK(hipEventRecord(e0, stream));
        CHECK(hipMemcpyAsync(plain, image, total, hipMemcpyDeviceToDevice, stream));
        CHECK(hipEventRecord(e1, stream));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (r >= 2) tc.push_back(ms);
    }
    std::sort(tm.begin(), tm.end());
    std::sort(tc.begin(), tc.end());
    const double m = tm[tm.size() / 2], c = tc[tc.size() / 2];
    std::printf("%llu commands, %llu bytes: mover %.3f ms (%.0f GB/s of payload, min %.3f max %.3f); hipMemcpyAsync device-to-device %.3f ms (%.0f GB/s, "
                "min %.3f max %.3f); the mover takes %.2fx the copy's time; the same bytes on the host link at 57 GB/s: %.3f ms\n",
                (ull)n, total, m, total / m * 1e-6, tm.front(), tm.back(), c, total / c * 1e-6, tc.front(), tc.back(), m / c, total / 57e9 * 1e3);
    return 0;
}
