// test_layout.cpp — csrc/layout.hpp on the CPU (no device code): the layout builder, pow2_at_least, the checked
// narrowings blocks_for / cub_count and the dense merges' two-halves grid (halves_of); and csrc/orset_layouts.hpp,
// the OR-Set wave path's carved blocks; and csrc/pnc_wave_layout.hpp, the PN-Counter wave's status block.  Prints one
// "ok <check>" line per check and "PASS" at the end; exits 1 at the first failure.  tests/test_layout.py runs it.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "layout.hpp"
#include "orset_layouts.hpp"
#include "pnc_wave_layout.hpp"

namespace jg {
struct Error {
    int code;
    std::string msg;
};
// the library's fail() (ctx.hip) throws its Error; so does this one
void fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    throw Error{code, buf};
}
}  // namespace jg

namespace {

int g_checks = 0;
#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);           \
            std::exit(1);                                                         \
        }                                                                         \
        ++g_checks;                                                               \
    } while (0)

template <class F> int code_of(F&& f) {
    try {
        f();
    } catch (const jg::Error& e) {
        return e.code;
    }
    return JG_OK;
}

struct Placed {
    size_t off, bytes, align;
};

// every combination of the counts and alignments, each as a 1-, 4- and 16-byte element, in one block
void test_layout() {
    struct E16 { uint64_t a, b; };
    const uint64_t counts[] = {0, 1, (1ull << 31) + 5};
    const size_t aligns[] = {8, 16, 256};
    jg::Layout L;
    std::vector<Placed> placed;
    uint8_t* p1[9];
    uint32_t* p4[9];
    E16* p16[9];
    int k = 0;
    CHECK(L.bytes() == 0);
    for (uint64_t c : counts)
        for (size_t a : aligns) {
            placed.push_back({L.add(p1[k], c, a), (size_t)c, a});
            placed.push_back({L.add(p4[k], c, a), (size_t)c * 4, a});
            placed.push_back({L.add(p16[k], c, a), (size_t)c * 16, a});
            ++k;
        }
    const size_t total = L.bytes();
    size_t prev_end = 0;
    for (const Placed& p : placed) {
        CHECK(p.off % p.align == 0);        // aligned as asked
        CHECK(p.off >= prev_end);           // in order, no overlap with the array before
        CHECK(p.off - prev_end < p.align);  // nothing but padding between them: a zero-count array takes no bytes
        CHECK(p.off + p.bytes <= total);    // the total covers it (a zero-count array's pointer is inside the block)
        prev_end = p.off + p.bytes;
    }
    CHECK(total >= prev_end && total - prev_end < 256 && total % 256 == 0);

    // bound to a base: typed pointers at the offsets; a zero-count array yields a usable (in-block, aligned) pointer;
    // bytes no array names are skipped; binding again moves every pointer
    uint32_t* a;
    uint64_t* z;
    uint8_t* b;
    jg::Layout M;
    CHECK(M.add(a, 3, 8) == 0 && M.skip(5) == 12 && M.add(z, 0, 256) == 256 && M.add(b, 1, 16) == 256);
    alignas(256) static unsigned char block[2][1024];
    CHECK(M.bytes() == 512);
    M.bind(block[0]);
    CHECK((void*)a == (void*)block[0] && (unsigned char*)z == block[0] + 256 && b == block[0] + 256);
    a[2] = 7, b[0] = 9;
    CHECK(block[0][8] == 7 && block[0][256] == 9);
    M.bind(block[1]);
    CHECK((void*)a == (void*)block[1] && b == block[1] + 256);

    // the default alignment is 256; a size that overflows size_t fails, and so does a 41st array
    uint8_t* d;
    uint64_t* big;
    jg::Layout D;
    D.add(d, 1);
    CHECK(D.add(d, 1) == 256);
    CHECK(code_of([&] { D.add(big, ~0ull / 4); }) == JG_EINVAL);
    CHECK(code_of([&] { for (int i = 0; i < 40; ++i) D.add(d, 1); }) == JG_EINVAL);
    std::printf("ok layout\n");
}

void test_round_pow2() {
    CHECK(jg::round_up(0, 256) == 0 && jg::round_up(1, 256) == 256 && jg::round_up(256, 256) == 256 && jg::round_up(257, 8) == 264);
    for (uint64_t floor : {64ull, 1024ull, 4096ull}) {
        CHECK(jg::pow2_at_least(0, floor) == floor);
        CHECK(jg::pow2_at_least(floor, floor) == floor);             // at its floor
        CHECK(jg::pow2_at_least(floor + 1, floor) == 2 * floor);
        CHECK(jg::pow2_at_least(1ull << 20, floor) == 1ull << 20);   // at a power of two
        CHECK(jg::pow2_at_least((1ull << 20) + 1, floor) == 1ull << 21);  // and one past it
    }
    std::printf("ok pow2_at_least\n");
}

void test_blocks_for() {
    for (unsigned block : {64u, 256u, 512u}) {
        CHECK(jg::blocks_for(0, block) == 1);  // clamped: one workgroup whose threads all fail their bounds check
        CHECK(jg::blocks_for(1, block) == 1);
        CHECK(jg::blocks_for(block, block) == 1);
        CHECK(jg::blocks_for(block + 1, block) == 2);
    }
    CHECK(jg::blocks_for(257) == 2);  // the default block is 256
    const uint64_t most = (uint64_t)INT32_MAX * 256;
    CHECK(jg::blocks_for(most) == (unsigned)INT32_MAX);
    CHECK(code_of([&] { jg::blocks_for(most + 1); }) == JG_EINVAL);        // 2^31 workgroups: fails
    CHECK(code_of([&] { jg::blocks_for((1ull << 40) * 256); }) == JG_EINVAL);  // would wrap to 0 in 32 bits
    CHECK(code_of([&] { jg::blocks_for(~0ull); }) == JG_EINVAL);           // n + block - 1 would wrap in 64 bits
    std::printf("ok blocks_for\n");
}

void test_cub_count() {
    CHECK(jg::cub_count(0) == 0);
    CHECK(jg::cub_count((uint64_t)INT32_MAX) == INT32_MAX);
    CHECK(code_of([&] { jg::cub_count((uint64_t)INT32_MAX + 1); }) == JG_EINVAL);
    std::string msg;
    try {
        jg::cub_count(1ull << 32, "ops");
    } catch (const jg::Error& e) {
        msg = e.msg;
    }
    CHECK(msg.find("4294967296 ops") != std::string::npos);  // the message names the count
    std::printf("ok cub_count\n");
}

// halves_of for the (cells per unit, units per workgroup) pairs the dense merge launches (csrc/pnc_dense.hip), held
// to the arithmetic written out: whole units, the cells past them, workgroups per half (at least one: a half's first
// workgroup owns the trailing cells), and whether both halves fit one launch.
void test_halves_of() {
    struct Shape { const char* name; uint32_t cells; uint64_t units; };
    const Shape shapes[] = {
        {"k_merge_dense<4>", 4, 256},             // a 16-B vector of int32 cells
        {"k_merge_dense<8>", 2, 256},             // of int64 cells
        {"k_merge_filtered, wide", 2, 512},       // kFiltCells, kFiltVecs x kFiltBlock
        {"k_merge_filtered, narrow", 2, 2 * 256},  // kNarrowCells, kNarrowVecs x kNarrowBlock
        {"k_merge_build", 2, 256},                // 2, kBuildBlock
    };
    for (const Shape& sh : shapes) {
        const uint64_t c = sh.cells, u = sh.units, group = c * u;  // one workgroup's cells
        const uint64_t most = 0x7FFFFFFFull * group + (c - 1);     // 2^31 - 1 workgroups per half and a full tail
        const uint64_t counts[] = {0, 1, c - 1, c, group - 1, group, group + 1, 3 * group + c + (c - 1), most, most + 1};
        for (uint64_t n : counts) {
            const jg::Halves h = jg::halves_of(n, sh.cells, sh.units);
            CHECK(h.n_units == n / c && h.tail == n % c && h.n_units * c + h.tail == n);
            const uint64_t covering = (n / c + u - 1) / u;
            CHECK(h.blocks == (covering ? covering : 1));
            CHECK(h.blocks * u >= h.n_units && (h.blocks - 1) * u <= h.n_units);
            CHECK(h.fits() == (n <= most));
        }
        CHECK(jg::halves_of(0, sh.cells, sh.units).blocks == 1 && jg::halves_of(c - 1, sh.cells, sh.units).tail == c - 1);
        CHECK(jg::halves_of(group, sh.cells, sh.units).blocks == 1 && jg::halves_of(group + 1, sh.cells, sh.units).blocks == 1);
        CHECK(jg::halves_of(group + c, sh.cells, sh.units).blocks == 2);
        CHECK(jg::halves_of(3 * group + c + (c - 1), sh.cells, sh.units).tail == c - 1 && c - 1 != 0);
        CHECK(jg::halves_of(most, sh.cells, sh.units).blocks == 0x7FFFFFFFull && jg::halves_of(most + 1, sh.cells, sh.units).blocks == 0x80000000ull);
    }
    // k_merge_dense's unit is a 16-B vector of eb-byte cells: the byte arithmetic its launch used before halves_of
    for (uint64_t eb : {4ull, 8ull})
        for (uint64_t n : {0ull, 1ull, 3ull, 4ull, 5ull, 15ull, 1023ull, 1024ull, 1025ull, 640000000ull, (1ull << 40) + 3}) {
            const jg::Halves h = jg::halves_of(n, (uint32_t)(16 / eb), 256);
            const uint64_t bytes = n * eb, nv = bytes / 16;
            CHECK(h.n_units == nv && h.tail == (bytes - nv * 16) / eb);
        }
    std::printf("ok halves_of\n");
}

// csrc/orset_layouts.hpp: the three carved blocks of the OR-Set wave path, held to their formulas written out
uint64_t al(uint64_t b) { return (b + 255) & ~255ull; }

// the fields the carve functions bind (the device structs Claims and Buckets hold the same ones)
struct Counts {
    uint32_t* scnt = nullptr;
    uint32_t* rcnt[2] = {nullptr, nullptr};
    unsigned long long* sbytes = nullptr;
};
struct Items {
    uint32_t *spos = nullptr, *sset = nullptr, *sitem = nullptr, *rpos = nullptr, *rset = nullptr;
    uint32_t* ritem[2] = {nullptr, nullptr};
};
template <class T> uint64_t off_of(const T* p, const void* base) { return (uint64_t)((uintptr_t)p - (uintptr_t)base); }

void test_orset_layouts() {
    // offsets of the large blocks are read against a base that is never dereferenced
    void* const far = reinterpret_cast<void*>(uintptr_t(1) << 40);
    // the claims' four count arrays of cap + 1 entries
    for (uint64_t cap : {0ull, 1ull, 62ull, 63ull, 1023ull, 1024ull, 1ull << 20, 0x7FFFFFF0ull - 1}) {
        Counts K, U;
        const uint64_t c4 = al((cap + 1) * 4);
        CHECK(jg::carve_claims(cap, far, K) == 3 * c4 + al((cap + 1) * 8));
        CHECK(off_of(K.scnt, far) == 0 && off_of(K.rcnt[0], far) == c4 && off_of(K.rcnt[1], far) == 2 * c4 && off_of(K.sbytes, far) == 3 * c4);
        CHECK(jg::carve_claims(cap, nullptr, U) == 3 * c4 + al((cap + 1) * 8) && U.scnt == nullptr && U.sbytes == nullptr);  // size only
    }
    {  // bound to a real block: the last entry of the last array lies inside it
        Counts K;
        std::vector<unsigned char> block(jg::carve_claims(62, nullptr, K));
        jg::carve_claims(62, block.data(), K);
        CHECK((void*)K.scnt == block.data());
        K.sbytes[62] = ~0ull;
        CHECK(off_of(K.sbytes, block.data()) + 63 * 8 <= block.size() && block[off_of(K.sbytes, block.data()) + 62 * 8] == 0xFF);
    }
    // the bucket commit's places and orders: three arrays per string-list entry, four per record-list entry
    for (uint64_t st_cap : {4096ull, 1ull << 20, 1ull << 30})
        for (uint64_t rt_cap : {4096ull, 1ull << 20, 1ull << 30}) {
            Items I;
            const uint64_t s4 = al((st_cap / 8) * 16 * 4 + 4), r4 = al((rt_cap / 8) * 16 * 4 + 4);
            CHECK(jg::carve_items(st_cap, rt_cap, far, I) == 3 * s4 + 4 * r4);
            CHECK(off_of(I.spos, far) == 0 && off_of(I.sset, far) == s4 && off_of(I.sitem, far) == 2 * s4);
            CHECK(off_of(I.rpos, far) == 3 * s4 && off_of(I.rset, far) == 3 * s4 + r4);
            CHECK(off_of(I.ritem[0], far) == 3 * s4 + 2 * r4 && off_of(I.ritem[1], far) == 3 * s4 + 3 * r4);
        }
    {
        Items I;
        std::vector<unsigned char> block(jg::carve_items(4096, 4096, nullptr, I));
        jg::carve_items(4096, 4096, block.data(), I);
        CHECK((void*)I.spos == block.data());
        I.ritem[1][(4096 / 8) * 16] = 1;  // the spare entry of the last array
        CHECK(off_of(I.ritem[1], block.data()) + ((4096 / 8) * 16 + 1) * 4 <= block.size());
    }
    static_assert(jg::kLists == 16, "the formulas above write kLists out");
    // the names staging: set | id | len | pad to 16 | pool offsets | pool bytes
    for (uint64_t n : {0ull, 1ull, 3ull, 4ull, 5ull})
        for (uint64_t nb : {0ull, 1ull, 17ull}) {
            const jg::NamesStaging L(n, nb);
            const uint64_t po = jg::round_up(12 * n, 16);
            CHECK(L.bytes == po + 8 * n + nb);
            CHECK(L.set == 0 && L.id == 4 * n && L.len == 8 * n && L.pool_off == po && L.pool == po + 8 * n);
        }
    {  // copy_out: three names whose bytes sit out of name order in the staged pool range [100, 117); one is empty
        const jg::NamesStaging L(3, 17);
        std::vector<unsigned char> h(L.bytes, 0);
        const uint32_t set[3] = {7, 7, 9}, id[3] = {0, 1, 5}, len[3] = {5, 0, 12};
        const uint64_t at[3] = {112, 105, 100};
        std::memcpy(h.data() + L.set, set, 12), std::memcpy(h.data() + L.id, id, 12), std::memcpy(h.data() + L.len, len, 12);
        std::memcpy(h.data() + L.pool_off, at, 24);
        std::memcpy(h.data() + L.pool, "twelve bytesAhell", 17);  // [100, 112) then [112, 117)
        uint32_t oset[3], oid[3];
        uint64_t off[4];
        unsigned char out[17];
        CHECK(L.copy_out(h.data(), 100, oset, oid, off, out) == 17);
        CHECK(std::memcmp(oset, set, 12) == 0 && std::memcmp(oid, id, 12) == 0);
        CHECK(off[0] == 0 && off[1] == 5 && off[2] == 5 && off[3] == 17);
        CHECK(std::memcmp(out, "Ahelltwelve bytes", 17) == 0);
        // no names: nothing written but off[0]
        off[0] = 9, off[1] = 9;
        CHECK(jg::NamesStaging(0, 0).copy_out(h.data(), 0, oset, oid, off, out) == 0 && off[0] == 0 && off[1] == 9);
    }
    std::printf("ok orset_layouts\n");
}

// csrc/pnc_wave_layout.hpp: the PN-Counter wave's status block — 64 bytes of status words, an 8-byte deferred mark
// per message from byte 64, a 4-byte roll-back slot per message from the next multiple of 16 past the marks of the
// capacity the block has — for blocks of exactly the bytes asked and of the bytes a growth allocates (half as much
// again: launch.hpp grow_keep)
struct WaveStatus {
    unsigned long long *status = nullptr, *deferred = nullptr;
    uint32_t* saved = nullptr;
};

void test_pnc_wave_layout() {
    void* const far = reinterpret_cast<void*>(uintptr_t(1) << 40);
    const uint64_t ns[] = {0, 1, 2, 3, 7, 8, 1000, 131072};
    const size_t kN = sizeof ns / sizeof ns[0];
    for (size_t k = 0; k < kN; ++k) {
        const uint64_t n = ns[k];
        const size_t need = 64 + n * 8 + n * 4 + 256;
        CHECK(jg::wave_status_bytes(n) == need);
        for (size_t bytes : {need, need + need / 2}) {
            const uint64_t cap = (bytes - 64 - 256) / 12;
            CHECK(jg::wave_status_capacity(bytes) == cap && cap >= n);  // the capacity read back covers what was asked
            WaveStatus w;
            const size_t end = jg::carve_wave_status(cap, far, w);
            CHECK(off_of(w.status, far) == 0 && off_of(w.deferred, far) == 64);
            CHECK(off_of(w.saved, far) == 64 + ((cap * 8 + 15) & ~15ull));
            CHECK(off_of(w.saved, far) >= 64 + cap * 8);                     // the slots start past the last mark
            CHECK(end == off_of(w.saved, far) + cap * 4 && end <= bytes);  // and end inside the block
        }
        // grown to hold the next size while `keep` messages' marks are live: what is carried over is the status words
        // and those marks, they lie inside the old block's list, and the new block's list starts where the old one did
        if (k + 1 < kN) {
            const size_t old_bytes = need + need / 2, grown = jg::wave_status_bytes(ns[k + 1]) + jg::wave_status_bytes(ns[k + 1]) / 2;
            const uint64_t old_cap = jg::wave_status_capacity(old_bytes);
            WaveStatus a, b;
            jg::carve_wave_status(old_cap, far, a);
            jg::carve_wave_status(jg::wave_status_capacity(grown), far, b);
            CHECK(off_of(b.deferred, far) == off_of(a.deferred, far) && off_of(b.status, far) == off_of(a.status, far));
            for (uint64_t keep : {(uint64_t)0, n}) {
                CHECK(jg::wave_status_keep(keep) == 64 + keep * 8);
                CHECK(jg::wave_status_keep(keep) <= off_of(a.deferred, far) + old_cap * 8);
                CHECK(jg::wave_status_keep(keep) <= off_of(b.saved, far));  // nothing carried over lands in the new slots
            }
        }
    }
    CHECK(jg::wave_status_capacity(0) == 0 && jg::wave_status_capacity(319) == 0 && jg::wave_status_capacity(320 + 11) == 0);
    {  // bound to a real block of the bytes a growth allocates: the last mark and the last slot lie inside it
        const size_t bytes = jg::wave_status_bytes(7) + jg::wave_status_bytes(7) / 2;
        const uint64_t cap = jg::wave_status_capacity(bytes);
        std::vector<unsigned char> block(bytes);
        WaveStatus w;
        jg::carve_wave_status(cap, block.data(), w);
        CHECK((void*)w.status == block.data());
        w.status[4] = ~0ull, w.deferred[cap - 1] = ~0ull, w.saved[cap - 1] = ~0u;
        CHECK(block[39] == 0xFF && block[64 + cap * 8 - 1] == 0xFF && block[off_of(w.saved, block.data()) + cap * 4 - 1] == 0xFF);
        WaveStatus u;
        CHECK(jg::carve_wave_status(cap, nullptr, u) <= bytes && u.status == nullptr && u.saved == nullptr);  // size only
    }
    std::printf("ok pnc_wave_layout\n");
}

}  // namespace

int main() {
    test_layout();
    test_round_pow2();
    test_blocks_for();
    test_cub_count();
    test_halves_of();
    test_orset_layouts();
    test_pnc_wave_layout();
    std::printf("PASS %d checks\n", g_checks);
    return 0;
}
