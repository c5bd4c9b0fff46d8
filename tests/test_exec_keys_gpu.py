"""GPU parity of the client batches by key name (jg_node_exec_keys, csrc/update.hip, csrc/pnc.hip).

Every batch is held to three yardsticks:
  (1) the sequential model (exec_keys_ref.ExecModel): the commands one by one, oracle_ref.pnc_apply_ops / pnc_values at
      the store's width, orset_names_ref.ORSetStr with the Interner;
  (2) reads deleted: a twin node takes the same batch without its reads through update_keys_ship.  The PN-Counter rows,
      the OR-Set records with their ords, the names log, the writes' outputs, their image bytes in order, sha and
      n_rounds must be equal (this also covers snap == 2);
  (3) cut into maximal runs: a second twin takes the batch as alternating update_keys_ship / query_keys calls (only
      where every snap is 0 or 1: the survivors of 2 are per call).  Every output including value and each command's
      snapshot bytes must be equal.
A command is (key, read, op, arg).
"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import janus_gpu as jg
import jsongen as J
from exec_keys_ref import ExecModel
from orset_names_ref import ADD, CLEAR, NEVER, NULL_ELEM, REMOVE
from test_query_keys_gpu import SHAPE_KEYS, World
from test_update_keys_gpu import DEC, INC, NA, pool, shuffled

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
ZERO32 = bytes(32)
Q_OK, Q_NO_KEY, Q_NO_CRDT, Q_OVERFLOW, Q_NO_ARG = jg.JG_Q_OK, jg.JG_Q_NO_KEY, jg.JG_Q_NO_CRDT, jg.JG_Q_OVERFLOW, jg.JG_Q_NO_ARG
NO_IDX = 0xFFFFFFFF
OUT = ("status", "result", "value", "kind", "idx", "elem", "guid")


def R_(key, arg=None):
    return (key, True, 0, arg)


def W_(key, op, arg=None):
    return (key, False, op, arg)


class Trio:
    """The node under test (a), the twin that gets the batch without its reads (b), the twin that gets it cut into runs
    (c), over one key space and the same cells, and the sequential model."""

    def __init__(self, ctx, rows=64, R=4, eb=8, pnc=True, orset=True, seed=1):
        self.a = World(ctx, rows, R, eb, pnc, orset, seed)
        self.b = World(ctx, rows, R, eb, pnc, orset, seed, ks=self.a.ks)
        self.c = World(ctx, rows, R, eb, pnc, orset, seed, ks=self.a.ks)
        self.worlds = (self.a, self.b, self.c)
        self.rng = np.random.default_rng(seed + 1000)
        self.m = ExecModel(self.a.guid, self.a.reg, self.a.P if pnc else None, self.a.N if pnc else None, null=NA, orset=orset)
        if pnc:  # row r gets 1 + r % R replicas, the same Guids on every node, so states differ in length
            guids = J.random_guids(np.random.default_rng(77), R)
            k = [r for r in range(rows) for _ in range(1 + r % R)]
            g = [guids[c] for r in range(rows) for c in range(1 + r % R)]
            for w in self.worlds:
                w.pnc.intern(k, [x[0] for x in g], [x[1] for x in g])

    def close(self):
        for w in (self.c, self.b, self.a):
            w.close()

    @property
    def ks(self):
        return self.a.ks

    def add_keys(self, keys, types, idx):
        gs = self.a.create(keys)
        for w in self.worlds:
            w.register(gs, types, idx)

    def reset_cells(self, P, N):
        self.m.P, self.m.N = P.copy(), N.copy()
        for w in self.worlds:
            w.write(P.copy(), N.copy())

    def stores(self, w):
        s = []
        if w.pnc is not None:
            s += [x.copy() for x in w.pnc.read_rows()]
        if w.ors is not None:
            s += [x.copy() for x in w.ors.read()] + [w.ors.names_since(0)]
        return s

    def run(self, cmds, snap=None, col=0, cut=True, n_rounds=None):
        n = len(cmds)
        keys, rd, ops, args = ([c[j] for c in cmds] for j in range(4))
        lo = self.rng.integers(1, 2**63, n, dtype=np.uint64)
        hi = self.rng.integers(0, 2**63, n, dtype=np.uint64)
        sn = None if snap is None else np.full(n, snap, np.uint8) if np.isscalar(snap) else np.asarray(snap, np.uint8)
        got = self.a.node.exec_keys(self.ks, keys, rd, ops, args, snap=sn, tags=(lo, hi), col=col, sha=True, with_guid=True)
        for name in OUT + ("snap_off", "n_bytes", "n_rounds"):  # printed before anything is asserted
            print(name, got[name] if n <= 16 or not isinstance(got[name], np.ndarray) else got[name][:16])

        # (1) the sequential model
        want = self.m.run(cmds, lo, hi, col)
        for name in OUT:
            assert np.array_equal(got[name], want[name]), (name, "model", np.flatnonzero(got[name] != want[name])[:8], got[name][:12], want[name][:12])
        reads = np.array(rd, bool)
        assert got["snap_off"].tolist() == [0] + np.cumsum([len(s) for s in got["states"]]).tolist() and got["n_bytes"] == int(got["snap_off"][-1])
        for i in np.flatnonzero(reads):
            assert got["states"][i] == b"" and got["sha"][i].tobytes() == ZERO32 and got["result"][i] == 0, (i, "a read ships nothing")
        assert not got["value"][~reads].any()
        if self.a.pnc is not None:
            P, N = self.a.pnc.read_rows()
            assert np.array_equal(P, self.m.P) and np.array_equal(N, self.m.N), "PN-Counter rows differ from the model's"
        if self.a.ors is not None and self.m.sets:
            sets = sorted(self.m.sets)
            assert self.a.ors.lookup_all_names(sets) == [self.m.sets[s].LookupAll() for s in sets]

        # (2) reads deleted
        w = np.flatnonzero(~reads)
        sub = lambda x: [x[i] for i in w]
        gb = self.b.node.update_keys_ship(self.ks, sub(keys), sub(ops), sub(args), snap=None if sn is None else sn[w], tags=(lo[w], hi[w]), col=col,
                                          sha=True, with_guid=True)
        for name in ("status", "result", "kind", "idx", "elem", "guid", "sha"):
            assert np.array_equal(got[name][w], gb[name]), (name, "reads deleted", np.flatnonzero(got[name][w] != gb[name])[:8])
        assert sub(got["states"]) == gb["states"] and got["n_bytes"] == gb["n_bytes"], "the image without the reads"
        assert got["n_rounds"] == gb["n_rounds"], (got["n_rounds"], gb["n_rounds"])
        if n_rounds is not None:
            assert got["n_rounds"] == n_rounds
        for x, y in zip(self.stores(self.a), self.stores(self.b)):
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, "stores, records with ords or names log differ from the twin's"

        # (3) cut into maximal runs (where it does not apply, the second twin takes the writes alone and stays in step)
        if not (cut and (sn is None or (sn[w] <= 1).all())):
            self.c.node.update_keys_ship(self.ks, sub(keys), sub(ops), sub(args), snap=None if sn is None else sn[w], tags=(lo[w], hi[w]), col=col)
        else:
            i = 0
            while i < n:
                j = i
                while j < n and rd[j] == rd[i]:
                    j += 1
                s = slice(i, j)
                if rd[i]:
                    elems = None if all(a is None for a in args[s]) else args[s]
                    value, status, kind, guid = self.c.node.query_keys(self.ks, keys[s], elems, with_guid=True)
                    for name, x in (("value", value), ("status", status), ("kind", kind), ("guid", guid)):
                        assert np.array_equal(got[name][s], x), (name, "cut", i, j)
                else:
                    gc = self.c.node.update_keys_ship(self.ks, keys[s], ops[s], args[s], snap=None if sn is None else sn[s], tags=(lo[s], hi[s]), col=col,
                                                      sha=True, with_guid=True)
                    for name in ("status", "result", "kind", "idx", "elem", "guid", "sha"):
                        assert np.array_equal(got[name][s], gc[name]), (name, "cut", i, j)
                    assert got["states"][s] == gc["states"], ("states", "cut", i, j)
                i = j
            if self.a.pnc is not None:
                for x, y in zip(self.a.pnc.read_rows(), self.c.pnc.read_rows()):
                    assert np.array_equal(x, y)
        return got


SET_KEYS = {b"set-0": 0, b"set-1": 1, b"set-2": 2, b"set-far": 5000}


def standing(ctx, eb, seed=None, **kw):
    """test_update_keys_gpu's standing world, on three nodes."""
    t = Trio(ctx, rows=64, R=4, eb=eb, seed=20 + eb if seed is None else seed, **kw)
    t.add_keys([b"pn-%d" % i for i in range(8)], [0] * 8, list(range(8)))
    types = [1 if i % 3 == 2 else 0 for i in range(len(SHAPE_KEYS))]
    t.add_keys(SHAPE_KEYS, types, [0 if ty else 8 + i for i, ty in enumerate(types)])
    t.add_keys(list(SET_KEYS), [1] * len(SET_KEYS), list(SET_KEYS.values()))
    t.add_keys([b"s-%d" % i for i in range(16)], [1] * 16, [10 + i for i in range(16)])
    t.a.create([b"created-only"])  # in the dictionary, never registered: NO_CRDT
    t.add_keys([b"pn-ovf"], [0], [40])  # a row whose checked Sum leaves the range: no test writes it
    P, N = t.m.P.copy(), t.m.N.copy()
    P[40] = np.iinfo(P.dtype).max
    t.reset_cells(P, N)
    return t


@pytest.fixture(scope="module")
def trios(ctx):
    ts = {eb: standing(ctx, eb) for eb in (4, 8)}
    yield ts
    for t in ts.values():
        t.close()


def mixed(n, seed):
    """test_update_keys_gpu's pool (every JG_U_* status, both kinds) with a read after every other command: of the same
    key with the same argument (so OR-Set reads carry strings, nulls and nothing, counter reads carry anything but an
    integer), and every 16th command a read of the row that overflows: every JG_Q_* status."""
    out = []
    for k, (key, op, arg) in enumerate(shuffled(pool(), n, seed)):
        if k % 16 == 5:
            out.append(R_(b"pn-ovf"))
        elif k % 2 == 0:
            out.append(W_(key, op, arg))
        else:
            out.append(R_(key, None if isinstance(arg, (int, np.integer)) else arg))
    return out


# ---- sizes and statuses -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_batch_sizes(trios, n):
    trios[8].run(mixed(n, 300 + n), snap=1 if n % 2 else None, col=3)


@pytest.mark.parametrize("eb", [4, 8])
@pytest.mark.parametrize("n", [64, 3000])
def test_every_status_and_kind_in_one_batch(trios, eb, n):
    cmds = mixed(n, 7 + n)
    got = trios[eb].run(cmds, snap=np.random.default_rng(n).integers(0, 3, n), col=eb % 3)  # snap 2 among them: yardsticks (1) and (2)
    rd = np.array([c[1] for c in cmds], bool)
    if n == 3000:
        assert set(got["status"][rd].tolist()) == {Q_OK, Q_NO_KEY, Q_NO_CRDT, Q_OVERFLOW, Q_NO_ARG} and set(got["status"][~rd].tolist()) == {0, 1, 2, 3, 4}
    else:  # one wave cannot hold the whole pool: the reads' OVERFLOW, and three codes at least over the wave
        assert Q_OVERFLOW in got["status"][rd].tolist() and len(set(got["status"].tolist())) >= 3
    assert set(got["kind"].tolist()) == {0, 1, 255}
    trios[eb].run(mixed(n, 11 + n), snap=np.random.default_rng(n + 1).integers(0, 2, n), col=1)  # snap 0 | 1: all three


# ---- PN-Counter reads -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eb", [4, 8])
def test_alternating_on_one_row_and_on_two(trios, eb):
    """257 commands alternating write / read on ONE row, then on two rows interleaved: the prefix crosses waves and
    workgroups through the sort and the scan by key.  P and N mixed, negative amounts, amounts that wrap the cell."""
    t = trios[eb]
    big = 2**31 - 5 if eb == 4 else 2**63 - 5
    amts = [3, -7, big, big, -big, 11, -(2**31) if eb == 4 else -(2**63), 2**40 + 1, 1]
    one = [R_(b"pn-0") if i % 2 else W_(b"pn-0", INC if (i // 2) % 3 else DEC, amts[(i // 2) % len(amts)]) for i in range(257)]
    got = t.run(one, snap=1, col=1)
    assert Q_OK in got["status"][1::2].tolist()
    two = []
    for i in range(257):
        k = (b"pn-1", b"pn-2")[(i // 2) % 2]
        two.append(R_(k, b"ignored") if i % 2 else W_(k, DEC if (i // 2) % 5 == 0 else INC, amts[(i // 3) % len(amts)]))
    t.run(two, snap=np.arange(257) % 2, col=2)
    # a read before any write of its row, and a read after the last
    t.run([R_(b"pn-3"), R_(b"pn-4"), W_(b"pn-3", INC, 9), W_(b"pn-4", DEC, 9), W_(b"pn-3", INC, -4), R_(b"pn-4"), R_(b"pn-3")], col=0)


@pytest.mark.parametrize("eb", [4, 8])
def test_overflow_appears_and_disappears_within_a_batch(ctx, eb):
    """col = 2 of R = 4: the changed cell lies inside the enumeration order."""
    t = Trio(ctx, rows=4, R=4, eb=eb, orset=False, seed=5)
    try:
        t.add_keys([b"k", b"other"], [0, 0], [1, 2])
        top = 2**31 - 1 if eb == 4 else 2**63 - 1
        dt = np.int32 if eb == 4 else np.int64
        P, N = np.zeros((4, 4), dt), np.zeros((4, 4), dt)
        P[1] = [top, 0, 0, 0]
        t.reset_cells(P, N)
        got = t.run([R_(b"k"), W_(b"k", INC, 1), R_(b"k")], col=2)
        assert got["status"].tolist() == [Q_OK, 0, Q_OVERFLOW] and got["value"].tolist() == [top, 0, 0]
        assert t.a.pnc.read_rows()[0][1].tolist() == [top, 0, 1, 0]  # the write is applied
        got = t.run([R_(b"k"), W_(b"k", INC, -1), R_(b"k"), R_(b"other")], col=2)
        assert got["status"].tolist() == [Q_OVERFLOW, 0, Q_OK, Q_OK] and got["value"].tolist() == [0, 0, top, 0]
        # the same through N, with a write on another row between
        N[1] = [0, top, 0, 0]
        t.reset_cells(P, N)
        got = t.run([W_(b"k", DEC, 1), W_(b"other", DEC, 5), R_(b"k"), W_(b"k", DEC, -1), R_(b"k"), R_(b"other")], col=2)
        assert got["status"].tolist() == [0, 0, Q_OVERFLOW, 0, Q_OK, Q_OK] and got["value"].tolist() == [0, 0, 0, 0, 0, -5]
    finally:
        t.close()


# ---- OR-Set reads -----------------------------------------------------------------------------------------------------
def test_one_name_through_add_remove_clear_add(trios):
    t, k = trios[8], b"s-0"
    cmds = [W_(k, ADD, b"x"), R_(k, b"x"), W_(k, REMOVE, b"x"), R_(k, b"x"), W_(k, CLEAR), R_(k, b"x"), W_(k, ADD, b"x"), R_(k, b"x"), R_(k, b"y"),
            R_(k, NA), R_(k)]
    got = t.run(cmds, snap=0)
    assert got["value"].tolist() == [0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0] and got["status"][-1] == Q_NO_ARG
    assert got["elem"].tolist() == [0, 0, 0, 0, 0, NEVER, 1, 1, NEVER, NULL_ELEM, NEVER]
    t.run(cmds, snap=1)  # the Clear now cuts a round under the reads
    t.run(cmds, snap=2)


def test_a_new_name_read_in_the_same_batch_and_by_a_whole_wave(trios):
    t = trios[8]
    got = t.run([R_(b"s-1", b"fresh"), W_(b"s-1", ADD, b"fresh"), R_(b"s-1", b"fresh"), R_(b"s-2", b"fresh")], snap=1)
    assert got["value"].tolist() == [0, 0, 1, 0] and got["elem"][1] == got["elem"][2] != NEVER and got["elem"][0] == NEVER
    # the Add closes one wave, its 64 reads fill the next exactly
    got = t.run([R_(b"pn-0")] * 63 + [W_(b"s-3", ADD, b"one new name")] + [R_(b"s-3", b"one new name")] * 64)
    assert got["value"][63:].tolist() == [0] + [1] * 64 and len(set(got["elem"][63:].tolist())) == 1


def test_the_null_element(trios):
    t, k = trios[4], b"s-4"
    got = t.run([R_(k, NA), W_(k, ADD, NA), R_(k, NA), W_(k, REMOVE, NA), R_(k, NA), W_(k, ADD, NA), R_(k, NA), R_(k, b"")])
    assert got["value"].tolist() == [0, 0, 1, 0, 0, 0, 1, 0] and (got["elem"][:7] == NULL_ELEM).all()


def test_membership_follows_the_walk_not_the_last_op(trios):
    """A repeated tag on a second Add: Add(t), Remove, Add(t) leaves the tag sets equal, so the element stays absent."""
    t, k = trios[8], b"s-5"
    n = 5
    lo, hi = np.array([77, 1, 2, 77, 3], np.uint64), np.array([5, 0, 0, 5, 0], np.uint64)
    cmds = [W_(k, ADD, b"rep"), W_(k, REMOVE, b"rep"), R_(k, b"rep"), W_(k, ADD, b"rep"), R_(k, b"rep")]
    keys, rd, ops, args = ([c[j] for c in cmds] for j in range(4))
    got = t.a.node.exec_keys(t.ks, keys, rd, ops, args, tags=(lo, hi), snap=np.zeros(n, np.uint8))
    want = t.m.run(cmds, lo, hi)
    print(got["value"], got["result"])
    assert got["value"].tolist() == want["value"].tolist() == [0, 0, 0, 0, 0] and got["result"].tolist() == want["result"].tolist() == [1, 1, 0, 1, 0]
    w = [0, 1, 3]  # the twins take the writes alone, so the three stay in step for the tests behind this one
    for tw in (t.b, t.c):
        tw.node.update_keys_ship(t.ks, [keys[i] for i in w], [ops[i] for i in w], [args[i] for i in w], tags=(lo[w], hi[w]), snap=np.zeros(3, np.uint8))
    for x, y in zip(t.stores(t.a), t.stores(t.b)):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y


def test_more_tombstones_than_adds_is_still_present(ctx):
    """A received state whose tombstone tags exceed its add tags for one element, then Remove, then a read: the sets of
    tags still differ, so the reference's !SetEquals keeps the element present."""
    t = Trio(ctx, rows=4, R=2, eb=8, seed=9)
    try:
        t.add_keys([b"odd"], [1], [3])
        add, rem = np.zeros(1, jg.REC_DTYPE), np.zeros(2, jg.REC_DTYPE)
        add["key"], add["tag_lo"], add["tag_hi"], add["ord"] = (3 << 32) | 0, 11, 1, 0
        rem["key"], rem["tag_lo"], rem["tag_hi"], rem["ord"] = (3 << 32) | 0, [21, 22], 1, [0, 1]
        for w in t.worlds:
            w.ors.load(add, rem)
            w.ors.names_sync([3], [1], [0], [(3, 0, b"el")])
        keys, rd, ops, args = [b"odd"] * 3, [1, 0, 1], [0, REMOVE, 0], [b"el", b"el", b"el"]
        lo, hi = np.ones(3, np.uint64), np.zeros(3, np.uint64)
        got = t.a.node.exec_keys(t.ks, keys, rd, ops, args, tags=(lo, hi), snap=np.zeros(3, np.uint8))
        print(got["value"], got["result"], got["elem"])
        assert got["value"].tolist() == [1, 0, 1] and got["result"].tolist() == [0, 1, 0] and got["elem"].tolist() == [0, 0, 0]
        gb = t.b.node.update_keys_ship(t.ks, [b"odd"], [REMOVE], [b"el"], tags=(lo[:1], hi[:1]), snap=[0])
        assert gb["result"].tolist() == [1]
        for x, y in zip(t.stores(t.a), t.stores(t.b)):
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
        v, st, _ = t.a.node.query_keys(t.ks, [b"odd"], [b"el"])
        assert v.tolist() == [1]
    finally:
        t.close()


def test_an_add_of_a_stored_tag_beside_a_read_of_its_element(ctx):
    """A tag repeated across calls.  The store holds (el, t).  Without a read, an Add of t on an element no Remove of the
    batch touches starts from an empty state: it issues a record and an ord, and the union drops the duplicate.  A read of
    that element in the batch must not change that: the records, their ords and the limits are the twin's, which never
    saw the read, and the read itself sees the stored tag."""
    t = Trio(ctx, rows=4, R=2, eb=8, seed=10)
    try:
        t.add_keys([b"k"], [1], [2])
        add = np.zeros(1, jg.REC_DTYPE)
        add["key"], add["tag_lo"], add["tag_hi"], add["ord"] = (2 << 32) | 0, 11, 1, 0
        for w in t.worlds:
            w.ors.load(add, np.zeros(0, jg.REC_DTYPE))
            w.ors.names_sync([2], [1], [0], [(2, 0, b"el")])
        lo, hi = np.array([5, 11, 33, 7], np.uint64), np.array([0, 1, 1, 0], np.uint64)
        keys, args = [b"k"] * 4, [b"el"] * 4
        got = t.a.node.exec_keys(t.ks, keys, [1, 0, 0, 1], [0, ADD, ADD, 0], args, tags=(lo, hi), sha=True)
        print(got["value"], got["result"], got["elem"], got["snap_off"])
        gb = t.b.node.update_keys_ship(t.ks, keys[1:3], [ADD, ADD], args[1:3], tags=(lo[1:3], hi[1:3]), sha=True)
        assert got["value"].tolist() == [1, 0, 0, 1] and got["result"].tolist() == [0, 1, 1, 0] and got["elem"].tolist() == [0] * 4
        assert got["states"][1:3] == gb["states"] and np.array_equal(got["sha"][1:3], gb["sha"]) and got["states"][0] == got["states"][3] == b""
        for x, y in zip(t.stores(t.a), t.stores(t.b)):
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, "records, ords or names differ from the twin's"
        assert len(t.a.ors.read()[0]) == 2
    finally:
        t.close()


def test_reads_land_in_rounds_0_and_1(trios):
    """A read between a shipping command and the Clear that cuts a round, and a read right after that Clear."""
    t, k = trios[8], b"s-6"
    got = t.run([W_(k, ADD, b"a"), R_(k, b"a"), W_(k, CLEAR), R_(k, b"a"), W_(k, ADD, b"b"), R_(k, b"b"), R_(k, b"a")], snap=1, n_rounds=2)
    assert got["value"].tolist() == [0, 1, 0, 0, 0, 1, 0]
    # reads alone between two Clears neither open nor cut a round
    t.run([W_(k, CLEAR), R_(k, b"b"), R_(k, NA), W_(k, CLEAR), R_(k, b"b")], snap=1, n_rounds=2)
    t.run([W_(k, ADD, b"c"), R_(k, b"c"), W_(k, CLEAR), R_(k, b"c")], snap=[0, 1, 0, 1], n_rounds=1)


# ---- reads only, writes only, one store -------------------------------------------------------------------------------
def test_reads_only_equals_query_keys_and_writes_nothing(trios):
    t = trios[8]
    t.run([W_(b"set-0", ADD, b"m"), W_(b"set-1", ADD, NA), W_(b"pn-0", INC, 5)])
    cmds = [c for c in mixed(600, 3) if c[1]]
    keys, args = [c[0] for c in cmds], [c[3] for c in cmds]
    before = t.stores(t.a)
    n = len(cmds)
    got = t.a.node.exec_keys(t.ks, keys, [1] * n, None, args, with_guid=True)  # op, amount, tags and snap NULL
    value, status, kind, guid = t.a.node.query_keys(t.ks, keys, args, with_guid=True)
    assert np.array_equal(got["value"], value) and np.array_equal(got["status"], status) and np.array_equal(got["kind"], kind)
    assert np.array_equal(got["guid"], guid) and got["n_bytes"] == 0 and got["n_rounds"] == 0 and not got["result"].any()
    assert {Q_OK, Q_NO_KEY, Q_NO_CRDT, Q_NO_ARG} <= set(status.tolist()) and value.any()  # (rows other tests drove out of range: OVERFLOW too)
    for x, y in zip(before, t.stores(t.a)):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, "a batch of reads wrote something"
    t.run(cmds)


def test_writes_only_equals_update_keys_ship(trios):
    cmds = [W_(*c) for c in shuffled(pool(), 300, 17)]
    got = trios[4].run(cmds, snap=np.random.default_rng(4).integers(0, 3, 300), col=2)
    assert got["n_bytes"] > 0 and not got["value"].any()


def test_nodes_with_one_store(ctx):
    for pnc, orset in ((True, False), (False, True)):
        t = Trio(ctx, rows=8, R=3, eb=8, pnc=pnc, orset=orset, seed=3)
        try:
            t.a.create([b"a", b"b", b"c"])
            gs = [t.a.guid[b"a"], t.a.guid[b"b"]]
            for w in t.worlds:
                w.register(gs, [0, 0] if pnc else [1, 1], [7, 0] if pnc else [0, 9])
            cmds = [W_(b"a", INC, 4), R_(b"a"), W_(b"b", DEC, 9), R_(b"b", b"x"), R_(b"c"), R_(b"d"), W_(b"a", ADD, b"x"), R_(b"a", b"x"), W_(b"b", ADD, NA),
                    R_(b"b", NA), W_(b"a", CLEAR), R_(b"a", b"x")] * 12
            got = t.run(cmds, snap=1, col=2 if pnc else 0)
            assert got["n_bytes"] > 0 and (got["n_rounds"] == 0) == pnc
            t.run([R_(b"c"), W_(b"d", INC, 1)], n_rounds=0)
        finally:
            t.close()


def test_tables_change_between_calls(ctx):
    """Registrations, a uid-table rehash, jg_pnc_reserve and an element-table rebuild between calls."""
    t = Trio(ctx, rows=16, R=3, eb=8, seed=8)
    try:
        t.add_keys([b"p0", b"s0"], [0, 1], [0, 0])
        probe = lambda: t.run([c for k in list(t.a.guid)[:40] + [b"absent"] for c in (W_(k, INC, 3), R_(k), W_(k, ADD, b"e0"), R_(k, b"e0"))], snap=1)
        probe()
        t.add_keys([b"p1", b"s1"], [0, 1], [5, 1])
        t.a.create([b"late"])
        assert probe()["status"][4 * 4 + 1] == Q_NO_CRDT
        g = [t.a.guid[b"late"]]
        for w in t.worlds:
            w.register(g, [0], [15])
        assert probe()["status"][4 * 4 + 1] == Q_OK
        for w in t.worlds:  # 3000 registrations: the uid table rehashes
            w.pnc.reserve(4000, 0)
        z = np.zeros((4000 - 16, 3), np.int64)
        t.m.P, t.m.N = np.vstack([t.m.P, z]), np.vstack([t.m.N, z])
        t.add_keys([b"bulk-%d" % i for i in range(3000)], [0] * 3000, list(range(16, 3016)))
        probe()
        for w in t.worlds:  # both dimensions: the reads sum rows of the new shape
            w.pnc.reserve(5000, 6)
        P, N = np.zeros((5000, 6), np.int64), np.zeros((5000, 6), np.int64)
        P[:4000, :3], N[:4000, :3] = t.m.P, t.m.N
        t.m.P, t.m.N = P, N
        t.add_keys([b"grown"], [0], [4999])
        got = t.run([W_(b"grown", INC, 11), R_(b"grown"), W_(b"p0", DEC, 4), R_(b"p0"), R_(b"bulk-2999"), W_(b"bulk-2999", INC, 1), R_(b"bulk-2999")], col=5)
        assert got["value"][1] == 11 and got["value"][6] - got["value"][4] == 1
        names = [b"name-%d" % i for i in range(6000)]  # a batch large enough to rebuild the element table
        t.run([W_((b"s0", b"s1")[i & 1], ADD, nm) for i, nm in enumerate(names)], snap=0)
        got = t.run([c for i, nm in enumerate(names[:150]) for c in (R_((b"s0", b"s1")[i & 1], nm), W_((b"s0", b"s1")[i & 1], REMOVE, nm),
                                                                    R_((b"s0", b"s1")[i & 1], nm))], snap=0)
        assert got["value"].tolist() == [1, 0, 0] * 150
    finally:
        t.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_and_stores_untouched(trios):
    t = trios[8]
    lib, p = jg.load(), jg._ptr
    cmds = [W_(b"pn-0", INC, 5), R_(b"pn-0"), W_(b"s-9", ADD, b"a name no call has interned"), R_(b"s-9", b"a name no call has interned"),
            W_(b"s-9", ADD, NA), R_(b"nope"), W_(b"s-9", CLEAR)]
    n = len(cmds)
    keys, rd, ops, args = ([c[j] for c in cmds] for j in range(4))
    koff, kdata, cmd, op, flag, amount, eoff, edata = jg.pack_exec(keys, rd, ops, args)
    lo, hi = np.arange(1, n + 1, dtype=np.uint64), np.arange(n, dtype=np.uint64)
    names = ("status", "result", "value", "kind", "idx", "elem", "guid")

    def call(node=t.a.node._h, koff=koff, cmd=cmd, op=op, flag=flag, amount=amount, eoff=eoff, lo=lo, col=0, snap=None, null=(), cap=1 << 16,
             want=jg.JG_EINVAL, stores=True, hi=hi, edata=edata, kdata=kdata, ks=t.ks._h, n_arg=n):
        o = {"status": np.full(n, 0xA5, np.uint8), "result": np.full(n, 0xA5, np.uint8), "value": np.full(n, -23, np.int64),
             "kind": np.full(n, 0xA5, np.uint8), "idx": np.full(n, 0xA5A5A5A5, np.uint32), "elem": np.full(n, 0xA5A5A5A5, np.uint32),
             "guid": np.full(2 * n, 0xA5A5A5A5A5A5A5A5, np.uint64), "snap_off": np.full(n + 1, 0xA5A5A5A5A5A5A5A5, np.uint64),
             "n_bytes": np.full(1, 0xA5A5A5A5A5A5A5A5, np.uint64), "out": np.full(1 << 16, 0xA5, np.uint8), "sha": np.full(32 * n, 0xA5, np.uint8),
             "n_rounds": np.full(1, 0xA5A5A5A5, np.uint32)}
        before, held = {k: v.copy() for k, v in o.items()}, t.stores(t.a) if stores else None
        sn = None if snap is None else np.asarray(snap, np.uint8)
        g = lambda k: None if k in null else p(o[k])
        rc = lib.jg_node_exec_keys(node, ks, n_arg, p(koff), p(kdata), p(cmd), p(op), p(flag), p(amount), p(eoff), p(edata), p(lo), p(hi), col, p(sn),
                                   *(g(k) for k in names), g("snap_off"), g("n_bytes"), g("out"), cap, g("sha"), g("n_rounds"))
        assert rc == want, (rc, want)
        if want != jg.JG_OK:
            for k in o:
                assert np.array_equal(o[k], before[k]), k
            if stores:
                for x, y in zip(held, t.stores(t.a)):
                    assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
        return o

    call(node=None)
    for name in ("status", "result", "value", "snap_off", "n_bytes", "out"):
        call(null=(name,))
    call(cmd=None)
    call(op=None)                                                      # the batch has writes
    call(koff=None)
    call(koff=np.array([0, 4, 3, 9, 13, 17, 20, 24], np.uint64))       # offsets that decrease
    call(cmd=np.array([0, 1, 0, 2, 0, 1, 0], np.uint8))                # a cmd above 1
    call(flag=np.array([3, 3, 1, 1, 2, 0, 0], np.uint8))               # a read that carries an integer
    call(flag=np.array([3, 0, 1, 4, 2, 0, 0], np.uint8))               # an arg_flag above 3
    call(amount=None)                                                  # a write carries an integer
    call(eoff=None)                                                    # a command carries a string
    call(lo=None)                                                      # a write carries an element
    call(hi=None)
    call(edata=None)
    call(kdata=None)
    call(ks=None)
    call(n_arg=(1 << 31) - 16)
    other = jg.Context(int(os.environ.get("JANUS_GPU_DEVICE", "0")))
    try:
        with jg.KeySpace(other, 8, 1 << 10) as ks2:                    # a key space and a node of different contexts
            call(ks=ks2._h)
    finally:
        other.close()
    call(col=4)
    call(snap=[1, 1, 1, 1, 3, 1, 1])                                   # a write's snap above 2
    jg._check(lib.jg_orset_wave_begin(t.a.ors._h, 1, 16))              # an open OR-Set wave holds the store
    try:
        call(stores=False)
    finally:
        jg._check(lib.jg_orset_wave_abort(t.a.ors._h))
    soff, nb, nr = np.full(1, 7, np.uint64), np.full(1, 7, np.uint64), np.full(1, 7, np.uint32)
    assert lib.jg_node_exec_keys(None, None, 0, *([None] * 10), 0, *([None] * 8), p(soff), p(nb), None, 0, None, p(nr)) == jg.JG_OK
    assert soff[0] == 0 and nb[0] == 0 and nr[0] == 0
    # a read's snap, op, tags and amount are ignored: garbage there is no refusal, and the arguments, unbroken, apply
    ok = call(snap=[1, 9, 1, 200, 1, 77, 1], want=jg.JG_OK)
    want = t.m.run(cmds, lo, hi, 0)
    for name in names[:-1]:
        assert np.array_equal(ok[name], want[name]), name
    assert int(ok["n_rounds"][0]) == 2 and int(ok["n_bytes"][0]) == int(ok["snap_off"][-1]) > 0
    w = [i for i in range(n) if not rd[i]]
    for tw in (t.b, t.c):
        tw.node.update_keys_ship(t.ks, [keys[i] for i in w], [ops[i] for i in w], [args[i] for i in w], tags=(lo[w], hi[w]))
    for x, y in zip(t.stores(t.a), t.stores(t.b)):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y


# ---- under hash collisions --------------------------------------------------------------------------------------------
def collision_scenario(ctx):
    t = standing(ctx, 8, seed=43)
    try:
        got = t.run(mixed(400, 12), snap=np.random.default_rng(1).integers(0, 2, 400))
        rd = np.array([c[1] for c in mixed(400, 12)], bool)
        assert set(got["status"][rd].tolist()) == {Q_OK, Q_NO_KEY, Q_NO_CRDT, Q_OVERFLOW, Q_NO_ARG} and set(got["status"][~rd].tolist()) == {0, 1, 2, 3, 4}
    finally:
        t.close()


def test_with_hash_collisions():
    """The test build's string hash keeps 4 bits: every probe chain is long.  In a child process through JANUS_GPU_LIB,
    as test_update_keys_gpu's."""
    lib = ROOT / "janus-crdt_amd" / "lib" / "libjanusgpu_test.so"
    assert lib.exists(), "the test build is made by __graft_entry__.build()"
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import janus_gpu as jg, test_exec_keys_gpu as t\n"
            "assert 'libjanusgpu_test' in str(jg.LIB_PATH)\n"
            "ctx = jg.Context(0)\nt.collision_scenario(ctx)\nctx.close()\nprint('PARITY OK')\n"
            % (str(ROOT / "janus-crdt_amd"), str(ROOT / "tests")))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240, env=dict(os.environ, JANUS_GPU_LIB=str(lib)),
                         cwd=str(ROOT / "tests"))
    assert out.returncode == 0 and "PARITY OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
