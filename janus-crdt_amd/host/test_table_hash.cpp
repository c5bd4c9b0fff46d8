// test_table_hash — csrc/table_hash.hpp on the CPU: no HIP, no library.  For every seed (command line, or one per
// line on stdin when there is none) it prints 1,000 lines "seq x h" with h = seq_hash(x) and 1,000 lines
// "uid lo hi h shard3" with h = uid_hash(lo, hi) and shard3 = shard_of_uid(lo, hi, 3), every number in hex.  The values
// come from splitmix64 of the seed; the first ones of each list are the edges (0, 1, all ones, one half zero).
// tests/test_table_hash.py holds tests/node_hash.py's Python restatements, which the GPU tests use to aim keys at a
// chosen slot, to these lines.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "table_hash.hpp"

namespace {

uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

constexpr int kValues = 1000;

void dump(uint64_t seed) {
    uint64_t s = seed;
    const uint64_t edge[] = {0, 1, ~0ull, 1ull << 63, 0xFFFFFFFFull, 1ull << 32, (1ull << 33) - 1, 0xFFFFFull};
    const int n_edge = (int)(sizeof(edge) / sizeof(edge[0]));
    for (int i = 0; i < kValues; ++i) {
        const uint64_t x = i < n_edge ? edge[i] : splitmix(s);
        std::printf("seq %" PRIx64 " %" PRIx64 "\n", x, jg::seq_hash(x));
    }
    for (int i = 0; i < kValues; ++i) {
        uint64_t lo = splitmix(s), hi = splitmix(s);
        if (i < n_edge) lo = edge[i];                      // with a random hi
        else if (i < 2 * n_edge) hi = edge[i - n_edge];    // with a random lo
        else if (i < 3 * n_edge) lo = edge[i - 2 * n_edge], hi = edge[(i + 3) % n_edge];
        std::printf("uid %" PRIx64 " %" PRIx64 " %" PRIx64 " %u\n", lo, hi, jg::uid_hash(lo, hi), jg::shard_of_uid(lo, hi, 3));
    }
}

}  // namespace

int main(int argc, char** argv) {
    std::vector<uint64_t> seeds;
    for (int i = 1; i < argc; ++i) seeds.push_back(std::strtoull(argv[i], nullptr, 0));
    if (argc < 2) {
        char line[128];
        while (std::fgets(line, sizeof line, stdin)) {
            char* end = nullptr;
            const uint64_t v = std::strtoull(line, &end, 0);
            if (end != line) seeds.push_back(v);
        }
    }
    if (seeds.empty()) {
        std::fprintf(stderr, "usage: test_table_hash SEED [SEED ...]   (or seeds on stdin, one per line)\n");
        return 2;
    }
    for (uint64_t seed : seeds) dump(seed);
    std::printf("PASS %zu seeds\n", seeds.size());
    return 0;
}
