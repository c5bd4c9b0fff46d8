// pnc_wave_layout.hpp — the PN-Counter wave's status block (jg::PncWave::stat, json.hip's wave_scratch), described
// once: 64 bytes of status words at 0, pass A's 8-byte deferred marks from 64, pass C's 4-byte roll-back slots after
// the marks at the capacity the block actually has, 256 spare bytes (they cover the padding in front of the slots).
// No HIP type: host/test_layout.cpp holds the offsets and sizes to the formulas written out there, with g++ alone.
#pragma once

#include "layout.hpp"

namespace jg {

constexpr size_t wave_status_bytes(uint64_t n) { return 64 + n * 12 + 256; }  // a block for n messages
// The messages a block of `bytes` holds (a block grows with head room: more than it was asked for).
constexpr uint64_t wave_status_capacity(size_t bytes) { return bytes < wave_status_bytes(0) ? 0 : (bytes - wave_status_bytes(0)) / 12; }
// What a growth carries over: the status words and the first `keep` marks (a streamed wave grows between chunks), at
// the same offsets in every block; the roll-back slots move with the capacity and are only written at finish time.
constexpr size_t wave_status_keep(uint64_t keep) { return 64 + keep * 8; }

// w.status, w.deferred and w.saved of a block with room for `cap` messages, bound to `base` if given.  Returns the
// end of the roll-back slots, which is inside the block.
template <class W> size_t carve_wave_status(uint64_t cap, void* base, W& w) {
    Layout L;
    L.add(w.status, 8, 64), L.add(w.deferred, cap, 8);
    const size_t saved = L.add(w.saved, cap, 16);
    if (base) L.bind(base);
    return saved + cap * 4;
}

}  // namespace jg
