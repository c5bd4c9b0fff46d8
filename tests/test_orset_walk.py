"""CPU-only: the OR-Set record walk in its prefix-sum form (tests/orset_walk_ref.py, the form csrc/orset_walk.hip
computes on the device) held to the oracle and to a sequential transcription of the host walk; the index arithmetic
of the kernels (csrc/orset_walk.hpp) under the sanitizers; the two new entry points in the library and the binding."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import janus_gpu as jg
import oracle_ref as orc
import orset_walk_ref as ref

ROOT = Path(__file__).resolve().parent.parent
BUILD = ROOT / "janus-crdt_amd" / "build"
NULL = ref.NULL_ELEM


def _state(rng, n_sets, n_elems, pool):
    """A stored state whose tombstones are not a subset of its adds, ords tied and out of tag order."""
    add, rem = [], []
    for s in range(n_sets):
        for e in list(range(n_elems)) + [NULL]:
            for t in pool:
                if rng.random() < 0.25:
                    add.append(((s << 32) | e, t[0], t[1], int(rng.integers(0, 6))))
                if rng.random() < 0.2:
                    rem.append(((s << 32) | e, t[0], t[1], int(rng.integers(0, 6))))
    return np.array(sorted(add), ref.REC_DTYPE), np.array(sorted(rem), ref.REC_DTYPE)


def _batch(rng, n, n_sets, n_elems, pool, reads):
    sets = rng.integers(0, n_sets, n).astype(np.uint32)
    elems = rng.integers(0, n_elems, n).astype(np.uint32)
    elems[rng.random(n) < 0.2] = NULL
    r = rng.random(n)
    ops = np.where(r < 0.08, 3, np.where(r < 0.55, 1, np.where((r < 0.8) | (not reads), 2, 4)))
    t = rng.integers(0, len(pool), n)
    lo = np.array([pool[k][0] for k in t], np.uint64)
    hi = np.array([pool[k][1] for k in t], np.uint64)
    return sets, elems, ops.astype(np.uint8), lo, hi


POOL = [(3, 9), (3, 4), (7, 1), (1, 8), (5, 5), (2, 2)]


def _same(x, y):
    return all(np.array_equal(a, b) for a, b in zip(x[:5], y[:5])) and x[5] == y[5]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_prefix_form_equals_the_sequential_walk(seed):
    """Reads included: results, records with ords, limits and Cleared sets, 1500 scripts per seed."""
    rng = np.random.default_rng(seed)
    for k in range(1500):
        A, R = _state(rng, 2, 2, POOL)
        b = _batch(rng, int(rng.integers(1, 24)), 2, 2, POOL, reads=True)
        assert _same(ref.walk_prefix(A, R, *b), ref.walk_sequential(A, R, *b)), (seed, k)


@pytest.mark.parametrize("seed", [11, 12])
def test_prefix_form_equals_the_oracle(seed):
    """Results, records and ords against ORSet.Add / Remove / Clear of the oracle, 1000 batches per seed over several
    sets with Clears, the null element, repeated tags and tombstones outside the add sets."""
    rng = np.random.default_rng(seed)
    for k in range(1000):
        A, R = _state(rng, 3, 2, POOL)
        b = _batch(rng, int(rng.integers(1, 30)), 3, 2, POOL, reads=False)
        res, adds, tombs, _, _, cleared = ref.walk_prefix(A, R, *b)
        ea, er, eres = orc.orset_apply_ops(A, R, *b)
        assert np.array_equal(res, eres), (seed, k)
        ga, gr = ref.union(A, R, adds, tombs, set(cleared))
        assert orc.same_orset(ga, gr, ea, er), (seed, k)


def test_limits_count_the_records_issued_so_far():
    A, R = _state(np.random.default_rng(5), 2, 2, POOL)
    b = _batch(np.random.default_rng(6), 40, 2, 2, POOL, reads=False)
    _, _, _, al, rl, _ = ref.walk_prefix(A, R, *b)
    order = sorted(range(40), key=lambda i: (int(b[0][i]), i))
    assert all(al[order[x]] <= al[order[x + 1]] and rl[order[x]] <= rl[order[x + 1]] for x in range(39))


@pytest.mark.parametrize("exe", ["test_orset_walk", "test_orset_walk_san"])
def test_kernel_index_arithmetic(exe):
    out = subprocess.run([str(BUILD / exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok" in out.stdout


def test_library_exports_the_walk_switch():
    lib = ctypes.CDLL(str(jg.LIB_PATH))
    assert hasattr(lib, "jg_orset_set_walk") and hasattr(lib, "jg_orset_walk_stats")
    assert lib.jg_abi_version() == 10


def test_binding_matches_the_header():
    src = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "janus_gpu.h").read_text(), flags=re.S)
    for name in ("jg_orset_set_walk", "jg_orset_walk_stats"):
        m = re.search(r"^\s*int\s+%s\s*\(([^)]*)\)" % name, src, flags=re.M)
        assert m, name
        assert name in jg.EXPORTS
        assert len(jg._SIGS[name][0]) == len(m.group(1).split(","))
    assert hasattr(jg.ORSetStore, "set_walk") and hasattr(jg.ORSetStore, "walk_stats")
