"""GPU: the one-launch form of the OR-Set record walk (csrc/orset_walk_small.hip) against the host walk.

Every batch goes to twin stores built identically, one pinned to the host walk (jg_orset_set_walk 0) and one to the
device walk with its one-launch form on (1 + jg_orset_set_walk_small 1).  After every call the results, the limits, both
record streams with their ords, the sizes, Contains of every touched element and LookupAll of every touched set must be
equal, the device twin must have copied no stored run to the host, and unless a case says otherwise its one-launch
counters must have advanced by exactly one batch and the batch's ops."""
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import janus_gpu as jg
import orset_walk_ref as ref
from orset_names_ref import ADD, CLEAR, REMOVE
from test_orset_walk_gpu import _long_run, _random, recs
from test_query_keys_gpu import World

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
NULL = jg.NULL_ELEM
A_, R_, C_ = 1, 2, 3
W = int(re.search(r"kThreads = (\d+);", (ROOT / "janus-crdt_amd" / "csrc" / "orset_walk_small.hpp").read_text()).group(1))  # the workgroup

_INTERNAL = (ROOT / "janus-crdt_amd" / "csrc" / "jg_internal.hpp").read_text()
AUTO_MIN = int(re.search(r"kWalkAutoMinOps = (\d+);", _INTERNAL).group(1))
SMALL_AUTO_MIN = int(re.search(r"kWalkSmallAutoMinOps = (\d+);", _INTERNAL).group(1))

ONE, MULTI, OVER, HOST = "one launch", "multi-launch", "over budget", "host"


def _moved(before, after):
    return {k: after[k] - before[k] for k in after}


class Twins:
    def __init__(self, ctx, add=(), rem=(), walk=1, small=1):
        self.h, self.d = jg.ORSetStore(ctx, 0, 0), jg.ORSetStore(ctx, 0, 0)
        self.h.set_walk(0)
        self.d.set_walk(walk)
        self.d.set_walk_small(small)
        self.keys = set()
        st = self.d.walk_small_stats()
        self.cap, self.max_stored = st["max_ops"], st["max_stored"]
        if len(add) or len(rem):
            for s in (self.h, self.d):
                s.load(recs(add), recs(rem))
            self.keys |= {int(k) for k in recs(add)["key"][:64]} | {int(k) for k in recs(rem)["key"][:64]}

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

    def apply(self, sets, elems, ops, lo=None, hi=None, route=ONE):
        n = len(ops)
        sets, elems, ops = np.asarray(sets, np.uint32), np.asarray(elems, np.uint32), np.asarray(ops, np.uint8)
        lo = np.arange(1, n + 1, dtype=np.uint64) if lo is None else np.asarray(lo, np.uint64)
        hi = np.zeros(n, np.uint64) if hi is None else np.asarray(hi, np.uint64)
        self.keys |= {(int(s) << 32) | int(e) for s, e, o in zip(sets, elems, ops) if o != 3}
        self.keys |= {(int(s) << 32) for s, o in zip(sets, ops) if o == 3}
        w0, s0, h0 = self.d.walk_stats(), self.d.walk_small_stats(), self.h.walk_stats()
        rh = self.h.apply_ops_ords(sets, elems, ops, lo, hi)
        rd = self.d.apply_ops_ords(sets, elems, ops, lo, hi)
        for name, x, y in zip(("result", "add_lim", "rem_lim"), rh, rd):
            print(name, x[:16], y[:16])
            assert np.array_equal(x, y), (name, np.flatnonzero(x != y)[:8])
        self.same_state()
        w, s = _moved(w0, self.d.walk_stats()), _moved(s0, self.d.walk_small_stats())
        print(route, w, s)
        hm = _moved(h0, self.h.walk_stats())
        assert (hm["device_batches"], hm["host_batches"], hm["device_ops"]) == (0, 1, 0)
        assert s["max_ops"] == 0 and s["max_stored"] == 0
        if route == HOST:
            assert (w["device_batches"], w["host_batches"], w["device_ops"]) == (0, 1, 0)
            assert (s["batches"], s["ops"], s["over_budget"]) == (0, 0, 0)
        else:
            assert w == {"device_batches": 1, "host_batches": 0, "device_ops": n, "run_bytes": 0}
            assert (s["batches"], s["ops"], s["over_budget"]) == {ONE: (1, n, 0), MULTI: (0, 0, 0), OVER: (0, 0, 1)}[route]
        return rh


@pytest.fixture
def twins(ctx):
    made = []

    def make(add=(), rem=(), **kw):
        made.append(Twins(ctx, add, rem, **kw))
        return made[-1]

    yield make
    for t in made:
        t.close()


def _union_at(old, new, cleared, base):
    """(the stream minus the Cleared sets) ∪ the batch's records, which take ords from `base` on."""
    have = {(int(r["key"]), int(r["tag_lo"]), int(r["tag_hi"])) for r in old}
    rows = [tuple(int(v) for v in r) for r in old if (int(r["key"]) >> 32) not in cleared]
    rows += [(int(r["key"]), int(r["tag_lo"]), int(r["tag_hi"]), int(r["ord"]) + base) for r in new
             if (int(r["key"]), int(r["tag_lo"]), int(r["tag_hi"])) not in have or (int(r["key"]) >> 32) in cleared]
    return np.array(sorted(rows), jg.REC_DTYPE)


def test_the_caps(twins):
    t = twins()
    assert t.cap >= 1024 and t.cap in (1024, 2048, 4096) and t.max_stored >= 1
    assert t.d.walk_small_stats() == {"batches": 0, "ops": 0, "over_budget": 0, "max_ops": t.cap, "max_stored": t.max_stored}


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, "W-1", "W", "W+1", "cap-1", "cap"])
def test_random_batches(twins, n, seed):
    """1. 5 sets x 7 elements, a 12-tag pool: keys, tags and epochs collide; three batches in a row on the growing state.
    11. For n <= 65 the results, limits and records also equal the Python model of the prefix-sum walk."""
    t = twins()
    n = {"W-1": W - 1, "W": W, "W+1": W + 1, "cap-1": t.cap - 1, "cap": t.cap}.get(n, n)
    rng = np.random.default_rng(100 * seed + n)
    for _ in range(3):
        b = _random(rng, n)
        A, R = t.d.read()
        rd = t.apply(*b, route=ONE if n <= t.cap else MULTI)  # (W + 1 is past a cap of W)
        if n <= 65:
            res, adds, tombs, al, rl, cleared = ref.walk_prefix(A, R, *b)
            assert np.array_equal(rd[0], res)
            base_a, base_r = int(rd[1][0]) - int(al[0]), int(rd[2][0]) - int(rl[0])
            assert np.array_equal(rd[1], al + np.uint64(base_a)) and np.array_equal(rd[2], rl + np.uint64(base_r))
            da, dr = t.d.read()
            assert np.array_equal(da, _union_at(A, adds, set(cleared), base_a))
            assert np.array_equal(dr, _union_at(R, tombs, set(cleared), base_r))


def test_past_the_cap(twins):
    """2. cap + 1 ops go to the multi-launch walk."""
    t = twins()
    rng = np.random.default_rng(5)
    t.apply(*_random(rng, t.cap + 1), route=MULTI)
    t.apply(*_random(rng, t.cap))


def test_one_segment_spans_the_batch(twins):
    """3. Every op on one (set, elem), Add and Remove alternating, a tag pool of 3: every wave and item boundary crossed."""
    t = twins()
    n = t.cap
    ops = [A_ if i % 2 == 0 else R_ for i in range(n)]
    lo = [1 + (i // 2) % 3 for i in range(n)]
    res = t.apply([3] * n, [4] * n, ops, lo=lo)
    assert res[0][1] == 1
    t.apply([3] * n, [4] * n, ops, lo=lo)


def test_no_segment_longer_than_one(twins):
    """4. cap ops on cap distinct sets, ids sparse up to 2^31, a Clear on the largest (the drop bitmap's size)."""
    t = twins()
    n = t.cap
    rng = np.random.default_rng(6)
    sets = np.unique(rng.integers(0, 2**31, 2 * n))[:n - 1].tolist() + [2**31]
    assert len(set(sets)) == n
    order = rng.permutation(n)
    sets = [sets[k] for k in order]
    t.apply(sets, [k % 3 for k in range(n)], [A_] * n)
    ops = [C_ if s == 2**31 else (R_ if k % 2 else A_) for k, s in enumerate(sets)]
    t.apply(sets, [k % 3 for k in range(n)], ops)
    t.apply([2**31, 2**31], [0, 0], [A_, R_])


@pytest.mark.parametrize("script", [
    ([C_, A_, A_, R_], "Clear first"),
    ([A_, A_, R_, C_], "Clear last"),
    ([A_, C_, A_, R_, C_, A_], "two Clears"),
    ([A_, R_, A_, C_, A_, R_, A_], "one tag on both sides of a Clear"),
    ([C_], "only a Clear"),
])
def test_clears(twins, script):
    """5. Clear first, last, twice; Adds and Removes of one tag on both sides of a Clear."""
    ops, what = script
    add = [((5 << 32) | 1, 3, 3, 0), ((5 << 32) | 1, 4, 4, 1), ((6 << 32) | 1, 1, 1, 0)]
    t = twins(add, add[:1])
    n = len(ops)
    lo = [3] * n if "one tag" in what else [3 + (i % 2) for i in range(n)]
    t.apply([5] * n, [1] * n, ops, lo=lo, hi=[3] * n if "one tag" in what else None)
    t.apply([6, 5, 5], [1, 1, 1], [R_, A_, R_], lo=[0, 3, 0])


def test_a_clear_in_every_set(twins):
    """5. Every set of the batch Cleared, with ops on both sides."""
    t = twins()
    rng = np.random.default_rng(7)
    t.apply(*_random(rng, 200))
    sets, elems, ops, lo, hi = _random(rng, 300)
    for s in range(5):
        ops[100 + s], sets[100 + s] = 3, s
    t.apply(sets, elems, ops, lo, hi)


def test_stored_runs(twins):
    """6. Tombstones that are not a subset of the adds, ords tied and descending against tag order; the batch Removes
    and re-Adds those keys (U0's (ord, tag) order in the first Remove's tombstones); an Add of a stored tag with no
    Remove of its key (the record and ord are issued, the union drops it)."""
    k1, k2, k3 = (1 << 32) | 2, (1 << 32) | 3, (2 << 32) | NULL
    add = [(k1, 10 + j, j % 2, (9 - j) // 2) for j in range(10)] + [(k2, 5, 0, 0), (k2, 6, 0, 0), (k3, 1, 1, 4), (k3, 2, 2, 4)]
    rem = [(k1, 12, 0, 3), (k1, 99, 9, 1), (k2, 7, 7, 0), (k3, 2, 2, 0)]
    t = twins(add, rem)
    t.apply([1, 1, 1], [2, 3, 3], [A_, A_, A_], lo=[10, 5, 8])  # stored tags added again, no Remove of the keys
    t.apply([1, 1, 1, 1, 2, 2, 1, 1], [2, 2, 2, 3, NULL, NULL, 3, 3], [R_, A_, R_, R_, R_, A_, A_, R_], lo=[0, 10, 0, 0, 0, 2, 7, 0],
            hi=[0, 0, 0, 0, 0, 2, 7, 0])
    t.apply([1, 1], [2, 2], [A_, R_], lo=[99, 0], hi=[9, 0])


def _run(key, n):
    return [(key, 10 + j, j % 3, (n - j) // 2) for j in range(n)] + [((1 << 32) | 0, 1, 1, 7), ((9 << 32) | 0, 1, 1, 2)]


def test_the_budget_edge(twins):
    """7. A stored add run of exactly kWalkSmallMaxStored tags under one Remove is walked in one launch; one more tag is
    not: the batch goes to the multi-launch walk with nothing written, twice in a row."""
    key = (2 << 32) | 1
    rows = _run(key, twins().max_stored)
    t = twins(rows, rows[3:9])
    res = t.apply([2, 2, 2], [1, 1, 1], [A_, R_, R_], lo=[5, 0, 0])
    assert list(res[0]) == [1, 1, 0] and res[2][1] - res[2][0] == t.max_stored - 6 + 1
    over = twins(_run(key, t.max_stored + 1), rows[3:9])
    res = over.apply([2, 2, 2, 1], [1, 1, 1, 0], [A_, R_, R_, A_], lo=[5, 0, 0, 3], route=OVER)
    assert list(res[0]) == [1, 1, 0, 1]
    over.apply([2, 2, 2, 1], [1, 1, 1, 0], [A_, R_, R_, A_], lo=[6, 0, 0, 3], route=OVER)
    over.apply([1, 1], [0, 0], [A_, R_])  # and the scratch is sound for the next one-launch batch


def test_non_dense_store(twins):
    """8. After a merge that deduplicated (chunks no longer full) and after Clears left chunks empty."""
    rows = _long_run()
    t = twins(rows[::2])
    t.each(lambda s: s.merge(recs(set(rows[1::2]) | set(rows[:200])), recs(rows[100:130])))
    t.same_state()
    big = [((100 + i // 40) << 32 | (i % 40), 1, 1, i) for i in range(8000)]
    t.each(lambda s: s.merge(recs(big), recs([])))
    t.apply(list(range(110, 280)), [0] * 170, [C_] * 170)
    res = t.apply([2, 2, 290, 2], [1, 1, 3, 1], [R_, A_, R_, R_], lo=[0, 4, 0, 0])
    assert list(res[0]) == [1, 1, 1, 1]
    t.apply([2, 150, 150, 105], [1, 3, 3, 3], [A_, A_, R_, R_], lo=[11, 1, 0, 0], hi=[1, 1, 0, 0])


def test_by_name_entry(ctx):
    """9. jg_orset_apply_ops_names on twins: 300 ops with repeated names and a Clear."""
    h, d = jg.ORSetStore(ctx, 0, 0), jg.ORSetStore(ctx, 0, 0)
    h.set_walk(0)
    d.set_walk(1)
    d.set_walk_small(1)
    try:
        rng = np.random.default_rng(9)
        names = [b"a", b"bb", b"ccc", None, b"dd"]
        for _ in range(3):
            n = 300
            sets = rng.integers(0, 4, n).astype(np.uint32)
            nm = [names[k] for k in rng.integers(0, len(names), n)]
            r = rng.random(n)
            ops = np.where(r < 0.03, 3, np.where(r < 0.6, 1, 2)).astype(np.uint8)
            ops[17] = 3
            lo, hi = rng.integers(1, 9, n).astype(np.uint64), np.zeros(n, np.uint64)
            x, y = h.apply_ops_names(sets, nm, ops, lo, hi, ords=True), d.apply_ops_names(sets, nm, ops, lo, hi, ords=True)
            for a, b in zip(x, y):
                assert np.array_equal(a, b)
            for a, b in zip(h.read(), d.read()):
                assert np.array_equal(a, b)
            assert h.names_since(0) == d.names_since(0)
            assert h.lookup_all_names([0, 1, 2, 3]) == d.lookup_all_names([0, 1, 2, 3])
        assert d.walk_stats() == {"device_batches": 3, "host_batches": 0, "device_ops": 900, "run_bytes": 0}
        s = d.walk_small_stats()
        assert (s["batches"], s["ops"], s["over_budget"]) == (3, 900, 0)
    finally:
        h.close()
        d.close()


def test_exec_keys_reads_among_the_writes(ctx):
    """10. jg_node_exec_keys on twin nodes: 200 commands, OR-Set reads among the writes, against the host-pinned node."""
    a = World(ctx, 16, 2, 8, False, True, 5)
    b = World(ctx, 16, 2, 8, False, True, 5, ks=a.ks)
    try:
        a.ors.set_walk(0)
        b.ors.set_walk(1)
        b.ors.set_walk_small(1)
        keys = [b"s-%d" % i for i in range(4)]
        gs = a.create(keys)
        for w in (a, b):
            w.register(gs, [1] * 4, [10, 11, 12, 13])
        rng = np.random.default_rng(3)
        args = [b"x", b"y", b"z", None]
        for _ in range(2):
            n = 200
            r = rng.random(n)
            ks_ = [keys[k] for k in rng.integers(0, 4, n)]
            rd = [bool(x < 0.35) for x in r]
            ops = [0 if x < 0.35 else (CLEAR if x < 0.38 else (ADD if x < 0.75 else REMOVE)) for x in r]
            ar = [None if o == CLEAR and not q else args[k] for o, q, k in zip(ops, rd, rng.integers(0, 4, n))]
            lo, hi = rng.integers(1, 40, n).astype(np.uint64), np.zeros(n, np.uint64)
            ga = a.node.exec_keys(a.ks, ks_, rd, ops, ar, tags=(lo, hi), sha=True, with_guid=True)
            gb = b.node.exec_keys(a.ks, ks_, rd, ops, ar, tags=(lo, hi), sha=True, with_guid=True)
            for name in ("status", "result", "value", "kind", "idx", "elem", "guid", "sha", "snap_off"):
                print(name, ga[name][:12], gb[name][:12])
                assert np.array_equal(ga[name], gb[name]), name
            assert ga["states"] == gb["states"]
            for x, y in zip(a.ors.read(), b.ors.read()):
                assert np.array_equal(x, y)
            assert a.ors.names_since(0) == b.ors.names_since(0)
        w, s = b.ors.walk_stats(), b.ors.walk_small_stats()
        assert w["run_bytes"] == 0 and w["host_batches"] == 0
        assert s["batches"] == w["device_batches"] >= 2 and s["ops"] == w["device_ops"] and s["over_budget"] == 0
        assert a.ors.walk_stats()["device_batches"] == 0
    finally:
        b.close()
        a.close()


CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import janus_gpu as jg
from test_orset_walk_small_gpu import Twins, _random
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
assert t.d.walk_small_stats()["batches"] == 16
t.close()
ctx.close()
print("RENUMBERED OK")
"""


def test_renumbering_under_a_low_ord_limit():
    """12. JANUS_TEST_ORD_LIMIT low enough that the unions renumber: a one-launch batch's limits are rebased like the
    twin's (a child process: the variable is read per call, the context is its own)."""
    env = dict(os.environ, JANUS_TEST_ORD_LIMIT="700")
    out = subprocess.run([sys.executable, "-c", CHILD % (str(ROOT / "janus-crdt_amd"), str(ROOT / "tests"))], capture_output=True, text=True,
                         timeout=300, env=env)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and "RENUMBERED OK" in out.stdout


def test_routing(twins):
    """13. The routing table of jg_orset_set_walk x jg_orset_set_walk_small, thresholds read from the source."""
    rng = np.random.default_rng(8)
    t = twins(walk=0, small=1)
    t.apply(*_random(rng, 500), route=HOST)
    t = twins(walk=2, small=0)
    t.apply(*_random(rng, 500), route=HOST if 500 < AUTO_MIN else MULTI)
    t = twins(walk=2, small=1)
    t.apply(*_random(rng, 500), route=ONE if 500 < AUTO_MIN else MULTI)
    assert t.cap + 1 < AUTO_MIN or AUTO_MIN <= t.cap
    t.apply(*_random(rng, t.cap + 1), route=HOST if t.cap + 1 < AUTO_MIN else MULTI)
    t.apply(*_random(rng, AUTO_MIN), route=MULTI)
    t = twins(walk=1, small=2)
    t.apply(*_random(rng, 500), route=MULTI)
    t = twins(walk=2, small=2)
    for n in sorted({1, 500, min(SMALL_AUTO_MIN, t.cap), t.cap}):
        auto_one = n < AUTO_MIN and SMALL_AUTO_MIN <= n <= t.cap
        t.apply(*_random(rng, n), route=ONE if auto_one else (HOST if n < AUTO_MIN else MULTI))
    with pytest.raises(jg.JanusError) as e:
        t.d.set_walk_small(3)
    assert e.value.code == jg.JG_EINVAL
    t.apply(*_random(rng, 500), route=ONE if SMALL_AUTO_MIN <= 500 < AUTO_MIN else (HOST if 500 < AUTO_MIN else MULTI))
    t = twins(walk=1, small=1)
    with pytest.raises(jg.JanusError):
        t.d.set_walk_small(-1)
    t.apply(*_random(rng, 64))  # the refused call changed nothing: still one launch
