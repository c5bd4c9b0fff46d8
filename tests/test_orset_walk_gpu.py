"""GPU: the OR-Set record walk on the device (csrc/orset_walk.hip) against the host walk it replaces.

Every batch goes to twin stores built identically, one pinned to the host walk (jg_orset_set_walk 0) and one to the
device walk (1).  After every call the results, the limits, both record streams with their ords, the sizes, Contains of
every touched element and LookupAll of every touched set must be equal, the device twin must have copied no stored run
to the host, and its op count must be the batch's."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import janus_gpu as jg
from orset_names_ref import ADD, CLEAR, REMOVE
from test_query_keys_gpu import World

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
NULL = jg.NULL_ELEM
A_, R_, C_ = 1, 2, 3


def recs(rows):
    return np.array(sorted(rows), jg.REC_DTYPE)


class Twins:
    def __init__(self, ctx, add=(), rem=(), modes=(0, 1)):
        self.h, self.d = jg.ORSetStore(ctx, 0, 0), jg.ORSetStore(ctx, 0, 0)
        self.h.set_walk(modes[0])
        self.d.set_walk(modes[1])
        self.keys, self.modes = set(), modes
        if len(add) or len(rem):
            for s in (self.h, self.d):
                s.load(recs(add), recs(rem))
            self.keys |= {int(k) for k in recs(add)["key"]} | {int(k) for k in recs(rem)["key"]}

    def close(self):
        self.h.close()
        self.d.close()

    def each(self, f):
        f(self.h)
        f(self.d)

    def same_state(self):
        (ha, hr), (da, dr) = self.h.read(), self.d.read()
        print("streams", len(ha), len(hr), len(da), len(dr))
        assert np.array_equal(ha, da), ("add stream", np.flatnonzero(ha != da)[:8] if ha.shape == da.shape else (ha.shape, da.shape))
        assert np.array_equal(hr, dr), ("tombstones", np.flatnonzero(hr != dr)[:8] if hr.shape == dr.shape else (hr.shape, dr.shape))
        assert self.h.size() == self.d.size() == (len(ha), len(hr))
        if self.keys:
            k = np.array(sorted(self.keys), np.uint64)
            s, e = (k >> np.uint64(32)).astype(np.uint32), (k & np.uint64(0xFFFFFFFF)).astype(np.uint32)
            assert np.array_equal(self.h.contains(s, e), self.d.contains(s, e))
            sets = np.unique(s)
            for x, y in zip(self.h.lookup_all(sets), self.d.lookup_all(sets)):
                assert np.array_equal(x, y)

    def apply(self, sets, elems, ops, lo=None, hi=None, host_runs=None):
        n = len(ops)
        sets, elems, ops = np.asarray(sets, np.uint32), np.asarray(elems, np.uint32), np.asarray(ops, np.uint8)
        lo = np.arange(1, n + 1, dtype=np.uint64) if lo is None else np.asarray(lo, np.uint64)
        hi = np.zeros(n, np.uint64) if hi is None else np.asarray(hi, np.uint64)
        self.keys |= {(int(s) << 32) | int(e) for s, e, o in zip(sets, elems, ops) if o != 3}
        self.keys |= {(int(s) << 32) for s, o in zip(sets, ops) if o == 3}
        before_h, before_d = self.h.walk_stats(), self.d.walk_stats()
        rh = self.h.apply_ops_ords(sets, elems, ops, lo, hi)
        rd = self.d.apply_ops_ords(sets, elems, ops, lo, hi)
        for name, x, y in zip(("result", "add_lim", "rem_lim"), rh, rd):
            print(name, x[:16], y[:16])
            assert np.array_equal(x, y), (name, np.flatnonzero(x != y)[:8])
        self.same_state()
        sh, sd = self.h.walk_stats(), self.d.walk_stats()
        if self.modes[1] == 1:
            assert sd["run_bytes"] == 0 and sd["host_batches"] == 0
            assert sd["device_batches"] == before_d["device_batches"] + 1 and sd["device_ops"] == before_d["device_ops"] + n
        assert sh["device_batches"] == 0 and sh["host_batches"] == before_h["host_batches"] + 1
        if host_runs is not None:
            assert (sh["run_bytes"] > before_h["run_bytes"]) == host_runs
        return rh


@pytest.fixture
def twins(ctx):
    made = []

    def make(add=(), rem=(), modes=(0, 1)):
        made.append(Twins(ctx, add, rem, modes))
        return made[-1]

    yield make
    for t in made:
        t.close()


def _random(rng, n, n_sets=5, n_elems=7, pool=12):
    sets = rng.integers(0, n_sets, n)
    elems = rng.integers(0, n_elems, n).astype(np.uint32)
    elems[rng.random(n) < 0.1] = NULL
    r = rng.random(n)
    ops = np.where(r < 0.04, 3, np.where(r < 0.6, 1, 2))
    t = rng.integers(1, pool + 1, n)
    return sets, elems, ops, t.astype(np.uint64), (t * 7 % 5).astype(np.uint64)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 3000])
def test_random_batches(twins, n, seed):
    """5 sets x 7 elements, a 12-tag pool: keys, tags and epochs collide; three batches in a row on the growing state."""
    rng = np.random.default_rng(100 * seed + n)
    t = twins()
    for _ in range(3):
        t.apply(*_random(rng, n))


def test_alternating_on_one_key(twins):
    n = 257
    t = twins()
    ops = [A_ if i % 2 == 0 else R_ for i in range(n)]
    res = t.apply([3] * n, [4] * n, ops, lo=[1 + (i // 2) % 5 for i in range(n)])
    assert res[0][1] == 1
    t.apply([3] * n, [4] * n, ops, lo=[1 + (i // 2) % 5 for i in range(n)], host_runs=True)


def test_many_sets_and_sparse_ids(twins):
    t = twins()
    sets = list(range(1000, 1300)) + [0, 7, 0xFFFFFFF0]
    n = len(sets)
    t.apply(sets, [i % 3 for i in range(n)], [A_] * n)
    t.apply(sets, [i % 3 for i in range(n)], [R_] * n, host_runs=True)
    t.apply([0xFFFFFFF0, 0xFFFFFFF0, 7], [0, NULL, 1], [A_, A_, R_])


def test_repeated_tag_in_an_epoch_and_after_a_clear(twins):
    t = twins()
    t.apply([1] * 7, [2] * 7, [A_, A_, R_, A_, C_, A_, A_], lo=[9, 9, 0, 9, 0, 9, 9])
    t.apply([1] * 4, [2, 2, 2, 2], [A_, R_, A_, R_], lo=[9, 0, 9, 0])


def test_stored_tag_added_again(twins):
    """With a Remove of the key in the batch the stored tag issues nothing; without one it issues a record and an ord the
    union drops: ords and limits equal the twin's either way."""
    add = [((1 << 32) | 2, 5, 0, 3), ((1 << 32) | 2, 6, 0, 1), ((1 << 32) | 3, 5, 0, 0)]
    t = twins(add)
    t.apply([1, 1, 1], [2, 3, 2], [A_, A_, A_], lo=[5, 5, 8], host_runs=False)
    t.apply([1, 1, 1, 1], [2, 3, 2, 2], [A_, A_, R_, A_], lo=[5, 5, 0, 6], host_runs=True)
    t.apply([1, 1, 1], [2, 2, 2], [A_, C_, R_], lo=[5, 0, 0])


def test_removes_that_find_nothing(twins):
    add = [((2 << 32) | 1, 4, 4, 0), ((2 << 32) | 1, 5, 5, 1)]
    t = twins(add, add)  # A == R
    res = t.apply([2, 2, 2, 2], [9, 1, 1, 9], [R_, R_, R_, R_])
    assert list(res[0]) == [0, 0, 0, 0]
    res = t.apply([2, 2, 2], [9, 9, 9], [A_, R_, R_])
    assert list(res[0]) == [1, 1, 0]


def test_presence_through_the_tombstones_outside_the_adds(twins):
    """More tombstones than adds: the element is present while a tombstone has no add (m > 0); an Add of that tag fills it."""
    k = (4 << 32) | 1
    t = twins([(k, 1, 0, 0)], [(k, 1, 0, 0), (k, 2, 0, 1)])
    res = t.apply([4] * 4, [1] * 4, [R_, A_, R_, R_], lo=[0, 2, 0, 0], host_runs=True)
    assert list(res[0]) == [1, 1, 0, 0]
    kn = (4 << 32) | NULL
    t2 = twins([], [(kn, 3, 0, 0)])
    res = t2.apply([4] * 3, [NULL] * 3, [R_, A_, R_], lo=[0, 3, 0])
    assert list(res[0]) == [1, 1, 0]


def test_null_element(twins):
    t = twins()
    res = t.apply([6] * 4, [NULL] * 4, [A_, R_, A_, R_], lo=[1, 0, 2, 0])
    assert list(res[0]) == [1, 1, 1, 1]
    t.apply([6] * 3, [NULL] * 3, [R_, A_, R_], lo=[0, 1, 0], host_runs=True)


def _long_run(n=3100):
    """One element's run across a 3072-slot chunk, ords descending in tag order, some tied."""
    k = (2 << 32) | 1
    rows = [(k, 10 + i, i % 3, (n - i) // 2) for i in range(n)]
    rows += [((1 << 32) | 0, 1, 1, 7), ((2 << 32) | 0, 1, 1, 9), ((2 << 32) | 2, 1, 1, 9), ((3 << 32) | 0, 1, 1, 2)]
    return rows


def test_long_stored_run(twins):
    rows = _long_run()
    t = twins(rows, rows[5:40])
    res = t.apply([2, 2, 2], [1, 1, 1], [A_, R_, R_], lo=[5, 0, 0], host_runs=True)
    assert list(res[0]) == [1, 1, 0]
    assert res[2][1] == res[2][2] and res[2][1] >= 3100 - 35


def test_long_stored_run_non_dense(twins):
    """The same after a merge that deduplicated (chunks no longer full) and after a Clear left chunks empty."""
    rows = _long_run()
    t = twins(rows[::2])
    t.each(lambda s: s.merge(recs(set(rows[1::2]) | set(rows[:200])), recs(rows[100:130])))
    t.same_state()
    big = [((100 + i // 40) << 32 | (i % 40), 1, 1, i) for i in range(8000)]
    t.each(lambda s: s.merge(recs(big), recs([])))
    t.apply(list(range(110, 280)), [0] * 170, [C_] * 170)
    res = t.apply([2, 2, 290, 2], [1, 1, 3, 1], [R_, A_, R_, R_], lo=[0, 4, 0, 0], host_runs=True)
    assert list(res[0]) == [1, 1, 1, 1]


@pytest.mark.parametrize("script", [
    ([C_, A_, A_, R_], "Clear first"),
    ([A_, A_, R_, C_], "Clear last"),
    ([A_, C_, A_, R_, C_, A_], "two Clears"),
    ([C_], "only a Clear"),
])
def test_clears(twins, script):
    ops, _ = script
    add = [((5 << 32) | 1, 3, 3, 0), ((5 << 32) | 1, 4, 4, 1), ((6 << 32) | 1, 1, 1, 0)]
    t = twins(add, add[:1])
    n = len(ops)
    t.apply([5] * n, [1] * n, ops, lo=[3 + (i % 2) for i in range(n)])
    t.apply([6, 5, 5], [1, 1, 1], [R_, A_, R_], lo=[0, 3, 0])


def test_limits_on_both_sides_of_a_clear(twins):
    add = [((5 << 32) | 1, 3, 3, 4), ((7 << 32) | 1, 3, 3, 2)]
    t = twins(add)
    sets = [7, 5, 5, 5, 5, 5, 7, 5]
    ops = [A_, A_, R_, C_, A_, R_, R_, A_]
    res, al, rl = t.apply(sets, [1] * 8, ops, lo=[9, 8, 0, 0, 8, 0, 0, 7])
    assert al[2] < al[4] and rl[2] < rl[5]  # ords issued before the Clear still count
    assert al[0] > al[7] - 1  # set 7 comes after set 5: its ords follow all of set 5's


def test_by_name_entry(ctx):
    """jg_orset_apply_ops_names on twins: results, ids, limits, records and the names log."""
    h, d = jg.ORSetStore(ctx, 0, 0), jg.ORSetStore(ctx, 0, 0)
    h.set_walk(0)
    d.set_walk(1)
    try:
        rng = np.random.default_rng(9)
        names = [b"a", b"bb", b"ccc", None, b"dd"]
        for _ in range(3):
            n = 300
            sets = rng.integers(0, 4, n).astype(np.uint32)
            nm = [names[k] for k in rng.integers(0, len(names), n)]
            r = rng.random(n)
            ops = np.where(r < 0.03, 3, np.where(r < 0.6, 1, 2)).astype(np.uint8)
            lo, hi = rng.integers(1, 9, n).astype(np.uint64), np.zeros(n, np.uint64)
            x, y = h.apply_ops_names(sets, nm, ops, lo, hi, ords=True), d.apply_ops_names(sets, nm, ops, lo, hi, ords=True)
            for a, b in zip(x, y):
                assert np.array_equal(a, b)
            for a, b in zip(h.read(), d.read()):
                assert np.array_equal(a, b)
            assert h.names_since(0) == d.names_since(0)
            assert h.lookup_all_names([0, 1, 2, 3]) == d.lookup_all_names([0, 1, 2, 3])
        assert d.walk_stats()["run_bytes"] == 0 and d.walk_stats()["device_batches"] == 3
        assert h.walk_stats()["run_bytes"] > 0
    finally:
        h.close()
        d.close()


def test_exec_keys_on_twin_nodes(ctx):
    """jg_node_exec_keys on nodes whose OR-Set stores are pinned each way: reads on keys with and without a Remove in
    the batch, a read after a Clear, a batch of reads only."""
    a = World(ctx, 16, 2, 8, False, True, 5)
    b = World(ctx, 16, 2, 8, False, True, 5, ks=a.ks)
    try:
        a.ors.set_walk(0)
        b.ors.set_walk(1)
        keys = [b"s-%d" % i for i in range(4)]
        gs = a.create(keys)
        for w in (a, b):
            w.register(gs, [1] * 4, [10, 11, 12, 13])
        Rd = lambda k, e: (k, True, 0, e)  # noqa: E731
        Wr = lambda k, o, e=None: (k, False, o, e)  # noqa: E731
        batches = [
            [Wr(b"s-0", ADD, b"x"), Wr(b"s-0", ADD, b"y"), Wr(b"s-1", ADD, b"x"), Wr(b"s-2", ADD, None)],
            [Rd(b"s-0", b"x"), Wr(b"s-0", REMOVE, b"x"), Rd(b"s-0", b"x"), Rd(b"s-0", b"y"), Wr(b"s-0", ADD, b"x"), Rd(b"s-0", b"x"),
             Rd(b"s-1", b"x"), Wr(b"s-1", ADD, b"z"), Rd(b"s-1", b"z"), Rd(b"s-2", None), Wr(b"s-2", REMOVE, None), Rd(b"s-2", None)],
            [Rd(b"s-1", b"x"), Wr(b"s-1", CLEAR), Rd(b"s-1", b"x"), Wr(b"s-1", ADD, b"x"), Rd(b"s-1", b"x"), Rd(b"s-1", b"z"), Rd(b"s-3", b"q")],
            [Rd(b"s-0", b"x"), Rd(b"s-0", b"y"), Rd(b"s-1", b"x"), Rd(b"s-2", None), Rd(b"s-3", b"x")],
        ]
        rng = np.random.default_rng(3)
        for cmds in batches:
            n = len(cmds)
            ks_, rd, ops, args = ([c[j] for c in cmds] for j in range(4))
            lo, hi = rng.integers(1, 2**63, n, dtype=np.uint64), rng.integers(0, 2**63, n, dtype=np.uint64)
            ga = a.node.exec_keys(a.ks, ks_, rd, ops, args, tags=(lo, hi), sha=True, with_guid=True)
            gb = b.node.exec_keys(a.ks, ks_, rd, ops, args, tags=(lo, hi), sha=True, with_guid=True)
            for name in ("status", "result", "value", "kind", "idx", "elem", "guid", "sha", "snap_off"):
                print(name, ga[name][:12], gb[name][:12])
                assert np.array_equal(ga[name], gb[name]), name
            assert ga["states"] == gb["states"]
            for x, y in zip(a.ors.read(), b.ors.read()):
                assert np.array_equal(x, y)
            assert a.ors.names_since(0) == b.ors.names_since(0)
        assert b.ors.walk_stats()["run_bytes"] == 0 and b.ors.walk_stats()["host_batches"] == 0
        assert a.ors.walk_stats()["device_batches"] == 0
    finally:
        b.close()
        a.close()


CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import janus_gpu as jg
from test_orset_walk_gpu import Twins, _random
ctx = jg.Context(0)
rng = np.random.default_rng(4)
t = Twins(ctx)
issued = 0
for step in range(16):
    b = _random(rng, 120, pool=4000)
    issued += int((b[2] == 1).sum())
    t.apply(*b)
a, r = t.d.read()
assert int(a["ord"].max()) < 700 and issued > 700, (int(a["ord"].max()), issued)  # so the unions did renumber
t.close()
ctx.close()
print("RENUMBERED OK")
"""


def test_renumbering_under_a_low_ord_limit():
    """JANUS_TEST_ORD_LIMIT low enough that the unions renumber: the limits are rebased by the store's next read after
    the renumbering, on both twins alike (a child process: the variable is read per call, the context is its own)."""
    env = dict(os.environ, JANUS_TEST_ORD_LIMIT="700")
    out = subprocess.run([sys.executable, "-c", CHILD % (str(ROOT / "janus-crdt_amd"), str(ROOT / "tests"))], capture_output=True, text=True,
                         timeout=300, env=env)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and "RENUMBERED OK" in out.stdout


def test_auto_mode_and_refusal(twins, ctx):
    t = twins(modes=(0, 2))
    rng = np.random.default_rng(8)
    t.apply(*_random(rng, 500))
    t.d.set_walk(2)
    before = t.d.walk_stats()
    t.apply(*_random(rng, 500))
    after = t.d.walk_stats()
    assert after["device_batches"] + after["host_batches"] == before["device_batches"] + before["host_batches"] + 1
    assert after["run_bytes"] == 0 or after["host_batches"] > before["host_batches"]
    t.apply(*_random(rng, 5000))  # past the auto threshold (kWalkAutoMinOps = 4096): on the device
    assert t.d.walk_stats()["device_batches"] == after["device_batches"] + 1
    with pytest.raises(jg.JanusError) as e:
        t.d.set_walk(3)
    assert e.value.code == jg.JG_EINVAL
    t.apply(*_random(rng, 64))  # the refused call changed nothing
