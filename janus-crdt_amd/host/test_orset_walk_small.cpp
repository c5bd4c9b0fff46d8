// test_orset_walk_small.cpp — csrc/orset_walk_small.hpp (the index arithmetic the one-launch OR-Set record walk adds
// to orset_walk.hpp's) on the CPU: no HIP, no library.  The packed upload's layout, the sort word of a stored item, the
// two segment-local loops and the packed sums are each held to a sequential restatement: sorting the words against
// sorting the (seg, ord, tag) records, the ranks against a sorted segment, first occurrences against a set.  Built
// twice (Makefile): plain, and under the address and undefined-behaviour sanitizers.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <set>
#include <tuple>
#include <vector>

#include "orset_walk_small.hpp"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t m) {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 33) % m);
}

int fails = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                                 \
        }                                                            \
    } while (0)

void test_caps() {
    CHECK(jgs::kMaxOps >= 1024 && jgs::kMaxOps <= jgs::kThreads);
    CHECK(jgs::kItemsPerThread * jgs::kThreads == jgs::kMaxStored);
    CHECK(jgs::item_key_bits(32) == 56 && jgs::item_key_bits(1) == 25);
    for (int b = 1; b <= 64; ++b) {
        const unsigned long long top = b == 64 ? ~0ull : (1ull << b) - 1;
        CHECK(jgs::bits_for(top) == b && jgs::bits_for(top >> 1) == (b == 1 ? 1 : b - 1));
    }
    CHECK(jgs::bits_for(0) == 1 && jgs::bits_for(1) == 1 && jgs::bits_for(2) == 2);
}

// The narrow sort word of an op orders like set << 32 | elem and gives it back.
void test_op_key() {
    for (int round = 0; round < 20000; ++round) {
        const uint32_t max_set = rnd(3) ? rnd(1u << (1 + rnd(16))) : 0xFFFFFFFFu - rnd(3), max_elem = rnd(3) ? rnd(100) : 0xFFFFFFFFu;
        const int sb = jgs::bits_for(max_set), eb = jgs::bits_for(max_elem);
        const uint32_t s1 = max_set ? rnd(max_set) + rnd(2) : 0, s2 = rnd(2) ? s1 : (max_set ? rnd(max_set) : 0);
        const uint32_t e1 = rnd(4) ? (max_elem ? rnd(max_elem) : 0) : max_elem, e2 = rnd(4) ? (max_elem ? rnd(max_elem) : 0) : max_elem;
        const unsigned long long k1 = jgs::op_key(s1, e1, eb), k2 = jgs::op_key(s2, e2, eb);
        const unsigned long long w1 = ((unsigned long long)s1 << 32) | e1, w2 = ((unsigned long long)s2 << 32) | e2;
        CHECK(jgs::op_key_wide(k1, eb) == w1 && jgs::op_key_wide(k2, eb) == w2);
        CHECK((k1 < k2) == (w1 < w2) && (k1 == k2) == (w1 == w2));
        CHECK(sb + eb == 64 || (k1 >> (sb + eb)) == 0);
    }
}

// The five arrays tile the block in order, each aligned to its element, and survive a round trip through one buffer.
void test_upload_layout() {
    for (uint64_t n : {1ull, 2ull, 3ull, 63ull, 64ull, 65ull, 1000ull, 1023ull, 1024ull}) {
        const jgs::Upload L = jgs::upload_layout(n);
        CHECK(L.lo == 0 && L.hi == L.lo + 8 * n && L.set == L.hi + 8 * n && L.elem == L.set + 4 * n && L.op == L.elem + 4 * n && L.bytes == L.op + n);
        CHECK(L.hi % 8 == 0 && L.set % 4 == 0 && L.elem % 4 == 0);
        std::vector<uint64_t> lo(n), hi(n);
        std::vector<uint32_t> set(n), elem(n);
        std::vector<uint8_t> op(n);
        for (uint64_t i = 0; i < n; ++i) lo[i] = rng_state + i, hi[i] = ~lo[i], set[i] = rnd(1u << 31), elem[i] = rnd(9), op[i] = (uint8_t)(1 + rnd(4));
        std::vector<uint64_t> block((L.bytes + 7) / 8);  // 8-byte aligned, exactly as long as the layout says
        char* b = reinterpret_cast<char*>(block.data());
        std::memcpy(b + L.lo, lo.data(), n * 8), std::memcpy(b + L.hi, hi.data(), n * 8), std::memcpy(b + L.set, set.data(), n * 4);
        std::memcpy(b + L.elem, elem.data(), n * 4), std::memcpy(b + L.op, op.data(), n);
        for (uint64_t i = 0; i < n; ++i) {
            CHECK(reinterpret_cast<const uint64_t*>(b + L.lo)[i] == lo[i] && reinterpret_cast<const uint64_t*>(b + L.hi)[i] == hi[i]);
            CHECK(reinterpret_cast<const uint32_t*>(b + L.set)[i] == set[i] && reinterpret_cast<const uint32_t*>(b + L.elem)[i] == elem[i]);
            CHECK(reinterpret_cast<const uint8_t*>(b + L.op)[i] == op[i]);
        }
    }
}

// Items of one key lie in tag order, key after key: sorting the words equals sorting (seg, ord, tag), dead items last.
void test_item_key() {
    for (int round = 0; round < 2000; ++round) {
        struct It { uint32_t seg, ord; unsigned long long lo, hi; uint32_t j; bool dead; };
        std::vector<It> items;
        uint32_t seg = rnd(3);
        while (items.size() < 60 && seg < jgs::kMaxOps) {
            std::set<std::pair<unsigned long long, unsigned long long>> tags;
            for (uint32_t k = rnd(9); k > 0; --k) tags.insert({rnd(4), rnd(4)});
            for (const auto& t : tags) {
                const uint32_t ord = rnd(3) ? rnd(4) : 0xFFFFFFFFu - rnd(2);
                items.push_back(It{seg, ord, t.first, t.second, (uint32_t)items.size(), rnd(4) == 0});
            }
            seg += 1 + rnd(400);
        }
        uint32_t max_ord = 0;
        for (const It& it : items) max_ord = std::max(max_ord, it.ord);
        const int ob = round % 3 == 0 ? 32 : jgs::bits_for(max_ord);
        std::vector<unsigned long long> words;
        for (const It& it : items) words.push_back(jgs::item_key(it.dead ? jgs::kItemNoSeg : it.seg, it.dead ? 0u : it.ord, it.j, ob));
        for (size_t x = 0; x < items.size(); ++x) {
            CHECK(jgs::item_idx(words[x]) == items[x].j);
            CHECK(jgs::item_seg(words[x], ob) == (items[x].dead ? jgs::kItemNoSeg : items[x].seg));
            CHECK(words[x] >> jgs::item_key_bits(ob) == 0);
        }
        std::sort(words.begin(), words.end());
        std::vector<It> live;
        for (const It& it : items)
            if (!it.dead) live.push_back(it);
        std::sort(live.begin(), live.end(), [](const It& a, const It& b) { return std::tie(a.seg, a.ord, a.lo, a.hi) < std::tie(b.seg, b.ord, b.lo, b.hi); });
        for (size_t x = 0; x < live.size(); ++x) CHECK(jgs::item_idx(words[x]) == live[x].j);
        for (size_t x = live.size(); x < words.size(); ++x) CHECK(jgs::item_seg(words[x], ob) == jgs::kItemNoSeg);
    }
    CHECK(jgs::item_idx(jgs::item_key(jgs::kMaxOps - 1, 0xFFFFFFFFu, jgs::kMaxStored - 1, 32)) == jgs::kMaxStored - 1);
    CHECK(jgs::item_seg(jgs::item_key(jgs::kMaxOps - 1, 0xFFFFFFFFu, jgs::kMaxStored - 1, 32), 32) == jgs::kMaxOps - 1);
}

// Positions in segments: first occurrences against a set per segment, ranks against the sorted flagged tags.
void test_segment_loops() {
    for (int round = 0; round < 4000; ++round) {
        const uint32_t n = 1 + rnd(40);
        std::vector<uint16_t> seg(n);
        std::vector<uint8_t> op(n), flag(n);
        std::vector<unsigned long long> lo(n), hi(n);
        for (uint32_t p = 0; p < n; ++p) {
            seg[p] = (uint16_t)((p == 0 || rnd(4) == 0) ? p : seg[p - 1]);
            op[p] = (uint8_t)(1 + rnd(4)), lo[p] = rnd(3), hi[p] = rnd(3), flag[p] = rnd(2);
        }
        std::set<std::tuple<uint32_t, unsigned long long, unsigned long long>> seen;
        for (uint32_t p = 0; p < n; ++p) {
            const auto k = std::make_tuple((uint32_t)seg[p], lo[p], hi[p]);
            CHECK(jgs::seen_before(op.data(), lo.data(), hi.data(), seg[p], p, lo[p], hi[p]) == (seen.count(k) != 0));
            if (op[p] == 1) seen.insert(k);
            uint32_t want = 0;
            for (uint32_t q = 0; q < n; ++q)
                if (seg[q] == seg[p] && flag[q] && std::make_pair(lo[q], hi[q]) < std::make_pair(lo[p], hi[p])) ++want;
            CHECK(jgs::rank_in_segment(flag.data(), seg.data(), lo.data(), hi.data(), n, seg[p], lo[p], hi[p]) == want);
        }
    }
}

void test_packed_sums() {
    for (int round = 0; round < 200; ++round) {
        const uint32_t n = round < 4 ? jgs::kMaxOps : 1 + rnd(jgs::kMaxOps);
        unsigned long long acc = 0;
        uint32_t is = 0, fl = 0, ua = 0;
        for (uint32_t p = 0; p < n; ++p) {
            CHECK(jgs::sum_is(acc) == is && jgs::sum_fl(acc) == fl && jgs::sum_ua(acc) == ua);  // the exclusive sums
            const bool i = round == 0 || rnd(2), f = i && (round == 1 || rnd(2));
            acc += jgs::pack3(i, f, i && !f);
            is += i, fl += f, ua += i && !f;
        }
        CHECK(jgs::sum_is(acc) == is && jgs::sum_fl(acc) == fl && jgs::sum_ua(acc) == ua);  // the block's total does not carry
    }
}

}  // namespace

int main() {
    test_caps();
    test_upload_layout();
    test_op_key();
    test_item_key();
    test_segment_loops();
    test_packed_sums();
    if (fails) {
        std::printf("%d checks failed\n", fails);
        return 1;
    }
    std::printf("orset_walk_small.hpp: ok\n");
    return 0;
}
