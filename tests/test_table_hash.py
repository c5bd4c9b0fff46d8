"""csrc/table_hash.hpp on the CPU: build/test_table_hash (host/test_table_hash.cpp, built by `make all` with g++) prints
seq_hash and uid_hash for 1,000 values per seed; build/test_table_hash_san is the same program under the address and
undefined-behaviour sanitizers, a stand-alone process.  tests/node_hash.py's Python restatements must equal those lines,
its inverses must invert them, and the shard rule must equal jg_shard_of: tests/test_node_tables_gpu.py aims uids and
identities at chosen slots of the device tables with them."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import node_hash as H

ROOT = Path(__file__).resolve().parents[1]


def _lines(name, seeds, stdin):
    exe = ROOT / "janus-crdt_amd" / "build" / name
    assert exe.exists(), "built by __graft_entry__.build()"
    if stdin:
        out = subprocess.run([str(exe)], input="".join("%d\n" % s for s in seeds), capture_output=True, text=True, timeout=60)
    else:
        out = subprocess.run([str(exe)] + [str(s) for s in seeds], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
    lines = out.stdout.split("\n")
    assert lines[-2] == "PASS %d seeds" % len(seeds), lines[-3:]
    seq = [tuple(int(v, 16) for v in ln.split()[1:]) for ln in lines if ln.startswith("seq ")]
    uid = [tuple(int(v, 16) for v in ln.split()[1:]) for ln in lines if ln.startswith("uid ")]
    assert len(seq) == len(uid) == 1000 * len(seeds) and len(seq) + len(uid) + 2 == len(lines)
    return seq, uid


@pytest.mark.parametrize("name,seeds,stdin", [("test_table_hash", [7], False), ("test_table_hash_san", [11], True),
                                              ("test_table_hash", [0, 2**64 - 1], True)])
def test_restatements_equal_the_header(name, seeds, stdin):
    """Every printed value, the edges among them (0, 1, all ones, a zero half on either side), through both builds and
    both ways of passing seeds."""
    seq, uid = _lines(name, seeds, stdin)
    assert (0, H.seq_hash(0)) in seq and any(lo == 0 and hi for lo, hi, _, _ in uid) and any(hi == 0 and lo for lo, hi, _, _ in uid)
    for x, h in seq:
        assert H.seq_hash(x) == h, hex(x)
        assert H.seq_unhash(h) == x, hex(x)
    for lo, hi, h, shard3 in uid:
        assert H.uid_hash(lo, hi) == h, (hex(lo), hex(hi))
        assert H.shard_of_uid(lo, hi, 3) == shard3
        assert H.uid_unhash(h, hi) == lo
        if lo == 0:
            assert H.uid_unhash_lo0(h) == hi
    assert len({h for _, h in seq}) == len({x for x, _ in seq})  # a bijection never folds two inputs


def test_inverses_hit_the_last_slot():
    """hash(unhash(h)) == h on 2,000 targets (j << 20) | 0xFFFFF: each homes to the last slot of every power-of-two table
    of up to 2^20 slots.  No identity comes out reserved (0 or 2^64 - 1) and no uid is Guid.Empty."""
    rng = np.random.default_rng(1)
    his = [int(v) for v in rng.integers(0, 2**64, 2000, dtype=np.uint64)]
    his[0], his[1], his[2] = 0, 1, 2**64 - 1
    for j in range(2000):
        h = H.last_slot_target(j)
        s = H.seq_unhash(h)
        assert H.seq_hash(s) == h and s not in (0, H.M64)
        lo = H.uid_unhash(h, his[j])
        assert H.uid_hash(lo, his[j]) == h and (lo, his[j]) != (0, 0)
        hi0 = H.uid_unhash_lo0(h)
        assert H.uid_hash(0, hi0) == h and hi0 != 0
        for cap in (1024, 4096, 1 << 20):
            assert h & (cap - 1) == cap - 1
    assert len(set(H.clustered_seqs(5, 300))) == 300
    us = H.clustered_uids(9, [None, 0] + his[3:40])
    assert us[0][0] == 0 and us[0][1] != 0 and us[1][1] == 0 and us[1][0] != 0


def test_shard_rule_equals_the_library():
    """(uid_hash >> 7) % world == jg_shard_of for worlds 2, 3, 5 and 8 (and rank 0 for a world of one): pure host
    arithmetic behind the C ABI, as tests/test_shard.py's owner rule."""
    sys.path.insert(0, str(ROOT / "janus-crdt_amd"))
    import janus_gpu as jg
    rng = np.random.default_rng(5)
    uids = [(int(a), int(b)) for a, b in rng.integers(0, 2**64, (300, 2), dtype=np.uint64)]
    uids += H.clustered_uids(0, [None, 0, 77]) + [(0, 1), (1, 0), (2**64 - 1, 2**64 - 1)]
    for world in (1, 2, 3, 5, 8):
        seen = set()
        for lo, hi in uids:
            r = jg.shard_of(lo, hi, world)
            assert r == (H.uid_hash(lo, hi) >> 7) % world == H.shard_of_uid(lo, hi, world)
            seen.add(r)
        assert seen == set(range(world))
