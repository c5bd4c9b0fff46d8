// layout.hpp — host-side sizing helpers that need no HIP type: rounding, pow2_at_least, the checked narrowings
// of a launch grid and of a hipcub item count, the two-halves grid of the dense PN-Counter merges, and the builder
// that carves one block into aligned arrays.
// launch.hpp adds the parts that touch a context or a stream; host/test_layout.cpp tests this file with g++ alone.
#pragma once

#include <climits>
#include <cstddef>
#include <cstdint>

#include "janus_gpu.h"

namespace jg {

[[noreturn]] void fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));  // ctx.hip

// x rounded up to a multiple of a (a power of two).
constexpr uint64_t round_up(uint64_t x, uint64_t a) { return (x + a - 1) & ~(a - 1); }

// The smallest floor << k that is >= x (floor a power of two: a power of two itself).
inline uint64_t pow2_at_least(uint64_t x, uint64_t floor) {
    uint64_t p = floor;
    while (p < x) p <<= 1;
    return p;
}

// Workgroups of `block` threads covering n items, at least one (a launch over zero items runs one workgroup whose
// threads all fail their bounds check).  A count that no launch can hold fails instead of wrapping.
inline unsigned blocks_for(uint64_t n, unsigned block = 256) {
    const uint64_t g = n / block + (n % block != 0);
    if (g > (uint64_t)INT_MAX) fail(JG_EINVAL, "%llu items in workgroups of %u exceed one launch (2^31 - 1)", (unsigned long long)n, block);
    return g ? (unsigned)g : 1u;
}

// The grid of a dense PN-Counter merge over n_cells cells per array (pnc_dense_kernels.hpp): two halves of `blocks`
// workgroups, P's then N's, each workgroup taking units_per_block units of cells_per_unit cells; a half's first takes
// the `tail` cells past the last whole unit, so a half has at least one.  fits(): both halves go into one launch.
struct Halves {
    uint64_t n_units;  // whole units per array
    uint32_t tail;     // trailing cells (< cells_per_unit)
    uint64_t blocks;   // workgroups per half (at least one)
    bool fits() const { return 2 * blocks < 0xFFFFFFFFull; }
};
inline Halves halves_of(uint64_t n_cells, uint32_t cells_per_unit, uint64_t units_per_block) {
    const uint64_t n_units = n_cells / cells_per_unit;
    const uint64_t blocks = n_units / units_per_block + (n_units % units_per_block != 0);
    return Halves{n_units, (uint32_t)(n_cells - n_units * cells_per_unit), blocks ? blocks : 1};
}

// A hipcub item count: hipcub's entry points are instantiated for int here.
inline int cub_count(uint64_t n, const char* what = "items") {
    if (n > (uint64_t)INT_MAX) fail(JG_EINVAL, "%llu %s exceed one hipcub call (2^31 - 1)", (unsigned long long)n, what);
    return (int)n;
}

// One block carved into arrays: add them in order, allocate bytes(), then bind() points each array into the block.
//     uint32_t* keys; uint64_t* vals;
//     Layout L;
//     L.add(keys, n), L.add(vals, n + 1, 8);
//     L.bind(<L.bytes() bytes, aligned to the largest alignment asked>);
// An array of zero elements takes no bytes beyond its padding and still gets a pointer inside the block.
class Layout {
public:
    // `count` elements at the next offset that is a multiple of `align` (a power of two); returns that offset.
    template <class T> size_t add(T*& p, uint64_t count, size_t align = 256) {
        const size_t off = skip(0, align);
        if (n_ == kMax || count > (SIZE_MAX - off) / sizeof(T))
            fail(JG_EINVAL, "scratch layout: array %d of %llu x %zu bytes does not fit", n_, (unsigned long long)count, sizeof(T));
        items_[n_++] = Item{&p, off, [](void* target, char* at) { *static_cast<T**>(target) = reinterpret_cast<T*>(at); }};
        end_ = off + count * sizeof(T);
        return off;
    }
    // `bytes` no array names (a staged copy, slack); returns their offset.
    size_t skip(uint64_t bytes, size_t align = 1) {
        const size_t off = round_up(end_, align);
        if (bytes > SIZE_MAX - off) fail(JG_EINVAL, "scratch layout: %llu bytes overflow", (unsigned long long)bytes);
        end_ = off + bytes;
        if (align > align_) align_ = align;
        return off;
    }
    // The block's size: the last array's end, rounded to the largest alignment (blocks then stack).
    size_t bytes() const { return round_up(end_, align_); }
    void bind(void* base) const {
        for (int i = 0; i < n_; ++i) items_[i].set(items_[i].target, static_cast<char*>(base) + items_[i].off);
    }

private:
    struct Item { void* target; size_t off; void (*set)(void* target, char* at); };
    static constexpr int kMax = 40;  // (jg_node_exec_keys carves 36)
    Item items_[kMax];
    size_t end_ = 0, align_ = 1;
    int n_ = 0;
};

}  // namespace jg
