// orset_wave.hpp — what the OR-Set wave path's files share: the constants, Tag16 and the sparse regions of pass 1
// (orset_wire.hip and its kernel headers orset_group.hpp, orset_tables.hpp, orset_commit.hpp), and the per-store
// state jg_orset_wire with its knobs (orset_wire.hip, which owns it; orset_encode.hip, which keeps its buffers there).
#pragma once

#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "launch.hpp"
#include "orset_layouts.hpp"
#include "orset_names.hpp"
#include "wire_cursor.hpp"

namespace {  // internal to each file that includes this, like the kernels that use it

using namespace jgn;  // the element table's layout and probes (orset_names.hpp)

constexpr int kBlock = 256;
constexpr unsigned long long kNone = ~0ull;
constexpr unsigned long long kKindState = 1, kKindInval = 2;  // error word = position << 2 | kind
constexpr uint32_t kDead = 0xFFFFFFFFu;                        // id of an entry at or beyond the limit

struct Tag16 { unsigned long long lo, hi; };

using jg::blocks_for;
using jg::ensure;
using jg::grow_keep;

// Pass 1 writes each message's entries and tags into SPARSE regions addressed by its byte offset, so
// no prefix over the wave is needed before parsing: an entry needs >= 5 payload bytes after an 11-byte
// `{"addSet":{` prefix and a tag >= 38 bytes, so message m's entries fit in slots [ceil(off/4),
// ceil(off_next/4)) and its tags in [ceil(off/32), ceil(off_next/32)) whatever the payload holds.
// check() compacts them in commit order (k_ow_compact).
constexpr uint64_t kEntryDiv = 4, kTagDiv = 32;

struct Sparse {  // entry slots: sort key, string offset, length | side << 31, error position, the string's
                 // first 8 bytes (zero past its end); tag slots
    unsigned long long* key;
    unsigned long long* noff;
    unsigned long long* pfx;
    uint32_t* meta;
    uint32_t* pos;
    uint32_t* set;             // the message's set
    uint32_t* sid;             // the string's slot in the wave's string table (k_ow_strings)
    unsigned long long* tref;  // null << 63 | side << 62 | the entry's parse-order ordinal in its message
    Tag16* tval;
    unsigned long long* trk;   // the record's identity without its tag (k_ow_rkeys): sid << 1 | side, or
                               // 1 << 63 | set << 1 | side for a null tag set
};

// The first index of `set` in snk, keys (set << 32 | ...) sorted ascending.
__device__ __forceinline__ uint64_t set_begin(const unsigned long long* snk, uint64_t n, uint32_t set) {
    uint64_t lo = 0, hi = n;
    const unsigned long long x = (unsigned long long)set << 32;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (snk[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint64_t rec_hash(unsigned long long k, const Tag16& g, uint32_t side) {
    return mix64(k ^ mix64(g.lo + side) ^ (g.hi * 0x9E3779B97F4A7C15ull));
}

}  // namespace

// The wave path's environment knobs (tests and A/B runs switch them between waves; unset or any other value = auto).
struct WaveKnobs {
    // JANUS_ORSET_TAIL: sort = the sort path alone; tables = no fall-back (the tables keep their certain bound, an
    // overflow is an error)
    enum Tail { kTailAuto, kTailSort, kTailTables } tail = kTailAuto;
    // JANUS_ORSET_PARSE: serial = the serial parse alone; group = the group parse alone (a message it leaves is rejected)
    enum Parse { kParseAuto, kParseSerial, kParseGroup } parse = kParseAuto;
    // JANUS_ORSET_COMMIT: radix = the radix path alone; buckets = no fall-back (a wave the bucket path cannot take is
    // an error); count = the bucket path with its counting pass always (never from the claims)
    enum Commit { kCommitAuto, kCommitRadix, kCommitBuckets, kCommitCount } commit = kCommitAuto;
    bool spec = true;    // JANUS_ORSET_SPEC=0: the commit packs and scans after the check (A/B runs)
    bool trace = false;  // JANUS_TRACE_MERGE (any value): host times of the check and the commit on stderr
    static WaveKnobs from_env() {
        const auto is = [](const char* e, const char* value) { return e && std::strcmp(e, value) == 0; };
        const char *t = std::getenv("JANUS_ORSET_TAIL"), *p = std::getenv("JANUS_ORSET_PARSE"), *c = std::getenv("JANUS_ORSET_COMMIT");
        WaveKnobs k;
        k.tail = is(t, "sort") ? kTailSort : is(t, "tables") ? kTailTables : kTailAuto;
        k.parse = is(p, "serial") ? kParseSerial : is(p, "group") ? kParseGroup : kParseAuto;
        k.commit = is(c, "radix") ? kCommitRadix : is(c, "buckets") ? kCommitBuckets : is(c, "count") ? kCommitCount : kCommitAuto;
        k.spec = !is(std::getenv("JANUS_ORSET_SPEC"), "0");
        k.trace = std::getenv("JANUS_TRACE_MERGE") != nullptr;
        return k;
    }
};

// The element table and the open wave of one store.
struct jg_orset_wire {
    jg::ElemTable names;  // the element table (orset_names.hpp)
    jg::DevBuf idcnt;  // per-set entry counts of the wave + two flag words (check_id_room's per-set tier)
    // open wave: payload, offsets, set per message, per-message counts / errors
    jg::DevBuf bytes, off, mset, ne, nt, na, err, eoff, toff, slow;  // slow: k_ow_group's per-message flags
    // the wave's payload / offsets / set ids: the buffers above (jg_orset_wave_*), or a node's
    // (csrc/node.hip: every kind's messages uploaded once, set id kSkipIdx for another kind's)
    uint8_t* vbytes = nullptr;
    uint64_t* voff = nullptr;
    uint32_t* vmset = nullptr;
    bool external = false;
    uint64_t wn = 0, wnb = 0, cap_msgs = 0, cap_bytes = 0;
    uint32_t max_set = 0;
    bool open = false, checked = false;
    // the first rejected message, with its error word's kind and byte position (read by the check: note_bad)
    uint64_t first_bad = ~0ull, bad_kind = 0, bad_pos = 0;
    uint64_t n_ent = 0, n_tag = 0;
    WaveKnobs knobs;  // read where the wave begins, where a chunk is parsed and where the commit starts
    // entries, groups, tags, records
    jg::DevBuf ekey, eval, enoff, emsg, emeta, epos, epfx, eset, skey, sval, hs, seg, impure, label, gid, eid;
    jg::DevBuf sp_key, sp_noff, sp_pfx, sp_meta, sp_pos, sp_set, sp_sid, sp_tref, sp_tval, sp_trk;  // pass 1's sparse regions (by byte offset)
    jg::DevBuf tref, tval, rkey, rside, dtab, dmin, dk[2], dt[2], ds[2], rk, rk2, perm[2], perm2[2];
    jg::DevBuf newk, newv, snk, snv, status, cub;
    jg::DevBuf cnk, fsel, fslot, fidx;  // commit: compacted new-string keys; dedup marks, slots, compacted indices
    jg_orset* recs = nullptr;  // a committed wave's records, sorted (the merge source), reused
    // key bits the entry sort orders on; tests narrow it (JANUS_TEST_ENTRY_SORT_BITS) so runs mix full keys
    int sort_bits = 32;
    // the wave's string and record tables (orset_tables.hpp), filled after each chunk's parse; `tables` =
    // they are being filled this wave, `tables_ok` = the check found them complete (no overflow)
    jg::DevBuf st_slot, st_list, rt_slot, rt_list, sid_id, ovf;  // 16-byte table slots (orset_tables.hpp); ovf: overflow word, sub-list counts
    jg::DevBuf st_packed, rt_packed, loffs;  // the sub-lists packed for the commit
    jg::DevBuf cb;                           // the bucket commit's places and bucket orders (jg::carve_items)
    // the bucket counts the tables' claimants take (jg::carve_claims; Claims, orset_tables.hpp): zeroed per wave for
    // cb_cap sets, and one place per string / record slot
    jg::DevBuf cbc, splace, rplace;
    uint64_t cb_cap = 0;
    // the check queued the commit's first steps ahead of its one read (lists packed, the claims' counts scanned:
    // spec_h = k_cb_scan's eight status words), for a commit of the whole wave from the tables
    bool spec = false;
    unsigned long long spec_h[9] = {};  // [8]: k_cb_scatter_claimed's bound flag (orset_commit.hpp)
    jg::DevBuf specst;
    uint64_t st_cap = 0, rt_cap = 0;     // slots in use this wave (a power of two, <= the allocations)
    uint64_t st_alloc = 0, rt_alloc = 0, seen_s = 0, seen_r = 0;  // allocated slots; the last checked wave's distinct strings / records
    bool tables = false, tables_ok = false;
    std::vector<unsigned long long> lc;  // host copy of ovf (overflow word, sub-list counts) taken by the check
    uint64_t last_cnt[2] = {0, 0};  // distinct records (add, tombstone) the last commit merged: the next wave's estimate
    jg::DevBuf enc_g, enc;       // jg_orset_encode_json (orset_encode.hip): the gathered records, the encoder's arrays
    jg::OrsetEncPlan enc_plan;   // its last size phase, for the write phase that follows
};
