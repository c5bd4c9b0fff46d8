"""GPU parity of the client writes by key name (jg_node_update_keys, csrc/update.hip).

Every batch is held to two yardsticks:
  * a Python model: a dict key -> guid, a dict guid -> (type, idx), oracle_ref.pnc_apply_ops for the PN-Counter cells at
    the store's width, orset_names_ref.ORSetStr per set and its Interner for the element ids; commands in batch order, the
    per-command status rules transcribed from PNCounterWrapper.Update and ORSetWrapper.Update (`rule` below);
  * a TWIN node driven the way a caller without this entry point drives it: KeySpace.lookup -> a Python dict ->
    PNCStore.apply_ops / ORSetStore.apply_ops_names.  After the batch the PN-Counter rows and values, the OR-Set records
    with their ords, encode_json's bytes, the names log, result, elem and the ord limits must all be equal.
"""
import ctypes as C
import os
import subprocess
import sys
import threading
from pathlib import Path

import numpy as np
import pytest

import janus_gpu as jg
import jsongen as J
import oracle_ref as orc
from orset_names_ref import ADD, CLEAR, NEVER, REMOVE, Interner, ORSetStr
from test_keyspace_gpu import entry, msg
from test_query_keys_gpu import KEY_LENS, SAME32, SHAPE_KEYS, World, key_of_len

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
NA = jg.NULL_ARG
OK, NO_KEY, NO_CRDT, BAD_ARG, BAD_OP = jg.JG_U_OK, jg.JG_U_NO_KEY, jg.JG_U_NO_CRDT, jg.JG_U_BAD_ARG, jg.JG_U_BAD_OP
NO_IDX = 0xFFFFFFFF
INC, DEC = 1, 2


def _b(x):
    return x.encode() if isinstance(x, str) else bytes(x)


def _is_int(a):
    return isinstance(a, (int, np.integer)) and not isinstance(a, bool)


def rule(t, op, arg):
    """The wrapper's verdict on (operationID, args) for a key of type t (0 PN-Counter, 1 OR-Set).
    PNCounterWrapper.Update (PNCounterWrapper.cs:33-48): `(int)args[0]` first (no argument or null: NullReference, a
    string: InvalidCast), then the switch (1 Increment, 2 Decrement, else InvalidOperation).
    ORSetWrapper.Update (ORSetWrapper.cs:30-47): the switch first (1 Add, 2 Remove, 3 Clear, else InvalidOperation); Add and
    Remove read `(string)args[0]` (a string or null; nothing or an int throws), Clear reads nothing."""
    if t == 0:
        if not _is_int(arg):
            return BAD_ARG
        return OK if op in (INC, DEC) else BAD_OP
    if op not in (ADD, REMOVE, CLEAR):
        return BAD_OP
    if op == CLEAR or arg is NA or isinstance(arg, (str, bytes)):
        return OK
    return BAD_ARG


class Duo:
    """A node written by key, its twin written the composed way, both over one key space, and the model of both."""

    def __init__(self, ctx, rows=64, R=4, eb=8, pnc=True, orset=True, seed=1):
        self.a = World(ctx, rows, R, eb, pnc, orset, seed)
        self.b = World(ctx, rows, R, eb, pnc, orset, seed, ks=self.a.ks)  # the same seed: the same cells
        self.b.guid = self.a.guid
        self.rng = np.random.default_rng(seed + 1000)
        self.P, self.N = (self.a.P.copy(), self.a.N.copy()) if pnc else (None, None)
        self.sets, self.it = {}, Interner()

    def close(self):
        self.b.close()
        self.a.close()

    @property
    def ks(self):
        return self.a.ks

    def add_keys(self, keys, types, idx, guids=None):
        gs = self.a.create(keys, guids)
        self.a.register(gs, types, idx)
        self.b.register(gs, types, idx)

    def reset_cells(self, P, N):
        self.P, self.N = P.copy(), N.copy()
        self.a.write(P, N)
        self.b.write(P, N)

    def tags(self, n):
        return self.rng.integers(1, 2**63, n, dtype=np.uint64), self.rng.integers(0, 2**63, n, dtype=np.uint64)

    def verdict(self, w, g, op, arg):
        """(status, kind, idx) of one command whose key resolved to guid g (None: the dictionary lacks it) on world w."""
        if g is None:
            return NO_KEY, 255, NO_IDX
        if g not in w.reg:
            return NO_CRDT, 255, NO_IDX
        t, ix = w.reg[g]
        st = rule(t, op, arg)
        return st, t, ix if st == OK else NO_IDX

    # ---- the model -----------------------------------------------------------------------------------------
    def model(self, cmds, lo, hi, col):
        n = len(cmds)
        out = {"status": np.zeros(n, np.uint8), "result": np.zeros(n, np.uint8), "kind": np.zeros(n, np.uint8), "idx": np.zeros(n, np.uint32),
               "elem": np.full(n, NEVER, np.uint32), "guid": np.zeros(n, jg.GUID_DTYPE)}
        rows, amt, isn = [], [], []
        for i, (k, op, arg) in enumerate(cmds):
            g = self.a.guid.get(_b(k))
            if g is not None:
                out["guid"][i] = g
            st, kd, ix = self.verdict(self.a, g, op, arg)
            out["status"][i], out["kind"][i], out["idx"][i] = st, kd, ix
            if st != OK:
                continue
            if kd == 0:
                rows.append(ix), amt.append(int(arg)), isn.append(op == DEC)
                out["result"][i] = 1
            else:
                name = None if (op == CLEAR or arg is NA) else _b(arg)
                out["result"][i] = 1 if self.sets.setdefault(ix, ORSetStr()).apply(op, name, (int(lo[i]), int(hi[i]))) else 0
                out["elem"][i] = self.it.op(ix, op, name)[0]
        if rows:
            self.P, self.N = orc.pnc_apply_ops(self.P, self.N, rows, [col] * len(rows), amt, isn)
        return out

    # ---- the twin: lookup -> dict -> apply_ops / apply_ops_names ------------------------------------------
    def composed(self, cmds, lo, hi, col):
        n = len(cmds)
        w = self.b
        out = {"status": np.zeros(n, np.uint8), "result": np.zeros(n, np.uint8), "elem": np.full(n, NEVER, np.uint32),
               "add_lim": np.zeros(n, np.uint64), "rem_lim": np.zeros(n, np.uint64)}
        found = w.ks.lookup([_b(c[0]) for c in cmds]) if n else []
        rows, amt, isn, oi, oset, oname, oop = [], [], [], [], [], [], []
        for i, ((k, op, arg), g) in enumerate(zip(cmds, found)):
            st, kd, ix = self.verdict(w, g, op, arg)
            out["status"][i] = st
            if st != OK:
                continue
            if kd == 0:
                rows.append(ix), amt.append(int(arg)), isn.append(op == DEC)
                out["result"][i] = 1
            else:
                oi.append(i), oset.append(ix), oop.append(op)
                oname.append(None if (op == CLEAR or arg is NA) else _b(arg))
        if oi:
            res, ids, al, rl = w.ors.apply_ops_names(oset, oname, oop, lo[oi], hi[oi], ords=True)
            out["result"][oi], out["elem"][oi], out["add_lim"][oi], out["rem_lim"][oi] = res, ids, al, rl
        if rows:
            w.pnc.apply_ops(rows, [col] * len(rows), amt, isn)
        return out

    def run(self, cmds, col=0, compare_stores=True):
        """cmds: [(key, op, arg)].  Returns update_keys' outputs after holding them to both yardsticks."""
        n = len(cmds)
        lo, hi = self.tags(n)
        got = self.a.node.update_keys(self.ks, [c[0] for c in cmds], [c[1] for c in cmds], [c[2] for c in cmds], tags=(lo, hi), col=col,
                                      with_guid=True, ords=True)
        m, c = self.model(cmds, lo, hi, col), self.composed(cmds, lo, hi, col)
        for name, want in m.items():
            assert np.array_equal(got[name], want), (name, "model", np.flatnonzero(got[name] != want)[:8])
        for name, want in c.items():
            assert np.array_equal(got[name], want), (name, "twin", np.flatnonzero(got[name] != want)[:8])
        if compare_stores:
            self.compare_stores()
        return got

    def compare_stores(self):
        a, b = self.a, self.b
        if a.pnc is not None:
            (P, N), (P2, N2) = a.pnc.read_rows(), b.pnc.read_rows()
            assert np.array_equal(P, P2) and np.array_equal(N, N2), "PN-Counter rows differ from the twin's"
            assert np.array_equal(P, self.P) and np.array_equal(N, self.N), "PN-Counter rows differ from the model's"
            for x, y in zip(a.pnc.values(), b.pnc.values()):
                assert np.array_equal(x, y)
        if a.ors is not None:
            for x, y in zip(a.ors.read(), b.ors.read()):
                assert np.array_equal(x, y)  # keys, tags and ords
            e1, l1 = a.ors.names_since(0)
            e2, l2 = b.ors.names_since(0)
            assert e1 == e2 == len(self.it.log) and l1 == l2 == self.it.log
            sets = sorted(self.sets)
            if sets:
                assert a.ors.encode_json(sets) == b.ors.encode_json(sets)
                names = a.ors.lookup_all_names(sets)
                assert names == [self.sets[s].LookupAll() for s in sets]


# ---- the standing world -----------------------------------------------------------------------------------------
SET_KEYS = {b"set-0": 0, b"set-1": 1, b"set-2": 2, b"set-far": 5000}


def standing(ctx, eb, seed=None):
    d = Duo(ctx, rows=64, R=4, eb=eb, seed=20 + eb if seed is None else seed)
    d.add_keys([b"pn-%d" % i for i in range(8)], [0] * 8, list(range(8)))
    types = [1 if i % 3 == 2 else 0 for i in range(len(SHAPE_KEYS))]  # every third key shape is an OR-Set key of set 0
    d.add_keys(SHAPE_KEYS, types, [0 if t else 8 + i for i, t in enumerate(types)])
    d.add_keys(list(SET_KEYS), [1] * len(SET_KEYS), list(SET_KEYS.values()))
    d.a.create([b"created-only"])  # in the dictionary, never registered: NO_CRDT
    return d


def pool():
    """Commands covering every status, both kinds and every precedence case."""
    c = [(b"pn-%d" % i, INC, 5 + i) for i in range(8)] + [(b"pn-%d" % i, DEC, -3 - i) for i in range(8)]
    c += [(b"pn-0", 3, None), (b"pn-0", 3, 7), (b"pn-1", INC, b"str"), (b"pn-1", DEC, NA), (b"pn-2", 0, 1), (b"pn-2", INC, None), (b"pn-3", 255, b"")]
    c += [(b"set-0", ADD, b"m"), (b"set-0", REMOVE, b"m"), (b"set-0", ADD, b"m2"), (b"set-0", ADD, b""), (b"set-0", CLEAR, None), (b"set-0", CLEAR, 5),
          (b"set-0", CLEAR, b"x"), (b"set-0", CLEAR, NA), (b"set-1", ADD, NA), (b"set-1", REMOVE, NA), (b"set-1", ADD, None), (b"set-1", REMOVE, 9),
          (b"set-0", 0, b"m"), (b"set-0", 4, NA), (b"set-0", 4, None), (b"set-2", ADD, "élément".encode()), (b"set-2", REMOVE, b"never"),
          (b"set-far", ADD, b"far"), (b"set-far", REMOVE, b"far")]
    c += [(k, ADD, b"shape") if i % 3 == 2 else (k, INC, 1) for i, k in enumerate(SHAPE_KEYS)]
    c += [(b"created-only", INC, 1), (b"created-only", ADD, b"x"), (b"no-such-key", INC, 1), (b"no-such-key", CLEAR, None), (b"pn-0\0", INC, 1),
          (b"\0", ADD, b"x"), (SAME32, INC, 1), (SAME32 + b"c", INC, 1), (b"prefi", INC, 1), (b"prefix-longer!", ADD, NA)]
    return c


def shuffled(cmds, n, seed):
    order = np.random.default_rng(seed).permutation(n)
    return [cmds[i % len(cmds)] for i in order]


@pytest.fixture(scope="module")
def duos(ctx):
    ds = {eb: standing(ctx, eb) for eb in (4, 8)}
    yield ds
    for d in ds.values():
        d.close()


@pytest.mark.parametrize("eb", [4, 8])
@pytest.mark.parametrize("n", [64, 3000])
def test_every_status_and_kind_in_one_batch(duos, eb, n):
    """Every status and both kinds shuffled into one wave and into a dozen workgroups: the ballot lists see arbitrary lane
    masks.  (64 commands cannot hold the whole pool: the wave-sized batch is asked for three statuses at least.)"""
    got = duos[eb].run(shuffled(pool(), n, 5 + n), col=eb % 3)
    if n >= len(pool()):
        assert set(got["status"].tolist()) == {OK, NO_KEY, NO_CRDT, BAD_ARG, BAD_OP}
    else:
        assert len(set(got["status"].tolist())) >= 3
    assert set(got["kind"].tolist()) == {0, 1, 255}
    bad = got["status"] != OK
    assert (got["result"][bad] == 0).all() and (got["idx"][bad] == NO_IDX).all() and (got["elem"][bad] == NEVER).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 3001])
def test_batch_sizes(duos, n):
    duos[8].run(shuffled(pool(), n, 100 + n), col=3)


def test_empty_batch(duos):
    d = duos[8]
    assert jg.load().jg_node_update_keys(None, None, 0, *([None] * 9), 0, *([None] * 8)) == jg.JG_OK
    d.run([])


@pytest.mark.parametrize("eb", [4, 8])
@pytest.mark.parametrize("n", [64, 257])
def test_hot_keys(duos, eb, n):
    """Every command of a batch on one address (and on two, interleaved): P and N mixed, negative amounts, and amounts
    that make the cell wrap at the store's width."""
    d = duos[eb]
    big = (1 << 31) - 1 if eb == 4 else (1 << 63) - 1
    amounts = [big, -7, 1, big, -big, 12345, -1, big - 3]
    one = [(b"pn-5", INC if i % 3 else DEC, amounts[i % len(amounts)]) for i in range(n)]
    before = d.P[5, 1]
    d.run(one, col=1)
    two = [((b"pn-6", b"pn-7")[i & 1], DEC if i % 5 < 2 else INC, amounts[(i * 3) % len(amounts)]) for i in range(n)]
    d.run(two, col=2)
    # the wrap is real: the exact sum of the P amounts leaves the cell's range
    exact = int(before) + sum(a for _, op, a in one if op == INC)
    info = np.iinfo(d.P.dtype)
    assert not info.min <= exact <= info.max and int(d.P[5, 1]) == (exact - info.min) % (1 << (8 * eb)) + info.min


def test_batches_of_one_kind(duos):
    d = duos[8]
    cmds = pool()
    d.run([c for c in cmds if not c[0].startswith(b"set-") and not (c[0] in SHAPE_KEYS and c[1] == ADD)] * 3)  # no OR-Set op
    d.run([c for c in cmds if not _is_int(c[2]) or c[0].startswith(b"set-")] * 3)                               # no PN-Counter op applies
    d.run([(b"set-0", CLEAR, None)] * 70)                                                                       # Clears alone


def test_clears_need_no_tags_or_elements(duos):
    """A batch whose OR-Set commands are all Clears without an element, beside PN-Counter commands: tags and elements NULL."""
    d = duos[8]
    cmds = [(b"set-1", ADD, b"to-clear")]
    d.run(cmds)
    cmds = [(b"pn-0", INC, 2), (b"set-1", CLEAR, None), (b"pn-1", DEC, 3), (b"set-1", CLEAR, 4)]
    got = d.a.node.update_keys(d.ks, [c[0] for c in cmds], [c[1] for c in cmds], [c[2] for c in cmds], tags=None, col=0)
    lo, hi = d.tags(len(cmds))
    m, c = d.model(cmds, lo, hi, 0), d.composed(cmds, lo, hi, 0)
    assert got["status"].tolist() == [OK] * 4 == m["status"].tolist() and got["result"].tolist() == [1] * 4 == c["result"].tolist()
    d.compare_stores()


def test_nodes_with_one_store(ctx):
    for pnc, orset in ((True, False), (False, True)):
        d = Duo(ctx, rows=8, R=3, eb=8, pnc=pnc, orset=orset, seed=3)
        try:
            d.a.create([b"a", b"b", b"c"])
            gs = [d.a.guid[b"a"], d.a.guid[b"b"]]
            for w in (d.a, d.b):
                w.register(gs, [0, 0] if pnc else [1, 1], [7, 0] if pnc else [0, 9])
            cmds = [(b"a", INC, 4), (b"b", DEC, 9), (b"c", INC, 1), (b"d", INC, 1), (b"a", ADD, b"x"), (b"b", ADD, NA), (b"a", REMOVE, b"x"),
                    (b"b", CLEAR, None), (b"a", 7, 1)] * 30
            got = d.run(cmds, col=2 if pnc else 0)
            want = [OK, OK, NO_CRDT, NO_KEY, BAD_ARG, BAD_ARG, BAD_ARG, BAD_ARG, BAD_OP] if pnc else \
                   [BAD_ARG, BAD_ARG, NO_CRDT, NO_KEY, OK, OK, OK, OK, BAD_OP]
            assert got["status"][:9].tolist() == want
            if not pnc:  # col is checked against a PN-Counter store only
                d.run(cmds[:9], col=1000)
        finally:
            d.close()


def test_precedence(duos):
    d = duos[4]
    cases = [((b"pn-0", 3, None), BAD_ARG), ((b"pn-0", 3, 7), BAD_OP), ((b"pn-0", 0, b"s"), BAD_ARG), ((b"pn-0", 0, NA), BAD_ARG), ((b"pn-0", 0, 0), BAD_OP)]
    cases += [((b"set-0", op, arg), BAD_OP) for op in (0, 4) for arg in (None, b"s", NA, 3)]
    cases += [((b"set-0", CLEAR, arg), OK) for arg in (None, b"s", NA, 3)]
    cases += [((b"set-0", op, arg), BAD_ARG) for op in (ADD, REMOVE) for arg in (None, 3)]
    d.run([(b"set-0", ADD, b"cleared-four-times")])
    got = d.run([c for c, _ in cases])
    assert got["status"].tolist() == [s for _, s in cases]
    assert got["result"].tolist() == [1 if s == OK else 0 for _, s in cases]  # a Clear returns true
    assert d.sets[0].LookupAll() == []


def test_orset_order(duos):
    d = duos[8]
    log0 = len(d.it.log)
    got = d.run([(b"set-2", ADD, b"w"), (b"set-2", REMOVE, b"w"), (b"set-2", CLEAR, None), (b"set-2", ADD, b"w"), (b"pn-0", INC, 1),
                 (b"set-2", REMOVE, b"not-live"), (b"set-2", ADD, NA), (b"set-2", REMOVE, NA), (b"set-2", REMOVE, NA)])
    assert got["result"].tolist() == [1, 1, 1, 1, 1, 0, 1, 1, 0]
    assert got["elem"][5] == NEVER and got["elem"][3] == got["elem"][0] + 1  # ids only grow, also across Clear
    assert [x[2] for x in d.it.log[log0:]] == [b"w", b"w"]  # the Remove of a name that is not live interned nothing
    log0 = len(d.it.log)
    got = d.run([(b"set-1", ADD, b"one new name, 64 times")] * 64)
    assert len(set(got["elem"].tolist())) == 1 and len(d.it.log) == log0 + 1 and (got["result"] == 1).all()
    assert d.sets[2].LookupAll() == [b"w"] and b"one new name, 64 times" in d.sets[1].LookupAll()


def key_scenario(d):
    """Key lengths 0 to 300, multi-byte keys, keys equal for 32 bytes, embedded NULs."""
    keys = sorted(set(key_of_len(n) for n in list(KEY_LENS) + list(range(0, 301, 13))) | set(SHAPE_KEYS))
    known = set(d.a.guid)
    new = [k for k in keys if k not in known]
    types = [i % 4 == 3 for i in range(len(new))]
    d.add_keys(new, [int(t) for t in types], [(1 + i % 3) if t else 30 + i for i, t in enumerate(types)])
    reg = d.a.reg
    cmds = []
    for k in keys:
        t = reg[d.a.guid[k]][0]
        cmds += [(k, ADD, b"by-" + k[:4]) if t else (k, INC, len(k) + 1), (k + b"\0", INC, 1), (k[:-1] + b"\0" if k else b"\0\0", ADD, b"x"), (k + b"x", INC, 1)]
    got = d.run(shuffled(cmds, len(cmds), 77))
    got = d.run(cmds)
    n = len(keys)
    assert (got["status"][0::4] == OK).all() and (got["status"][1::4] == NO_KEY).all() and (got["status"][2::4] == NO_KEY).all()
    return n


def test_key_shapes(duos):
    assert key_scenario(duos[8]) > 30


def collision_scenario(ctx):
    """The key shapes and 200 keys in 16 probe chains, every status, against the model and the twin."""
    d = standing(ctx, 8, seed=41)
    try:
        key_scenario(d)
        keys = [b"key-%03d" % i for i in range(200)]
        d.a.pnc.reserve(400, 0), d.b.pnc.reserve(400, 0)
        z = np.zeros((400 - 64, 4), np.int64)
        d.P, d.N = np.vstack([d.P, z]), np.vstack([d.N, z])
        types = [i % 4 == 3 for i in range(200)]
        d.add_keys(keys, [int(t) for t in types], [(i % 5) if t else 150 + i for i, t in enumerate(types)])
        cmds = [(k, ADD if t else INC, b"el-%d" % (i % 9) if t else i) for i, (k, t) in enumerate(zip(keys, types))]
        cmds += [(k, REMOVE if t else DEC, b"el-%d" % (i % 7) if t else -i) for i, (k, t) in enumerate(zip(keys, types))]
        cmds += pool()
        got = d.run(shuffled(cmds, 2 * len(cmds), 12))
        assert set(got["status"].tolist()) == {OK, NO_KEY, NO_CRDT, BAD_ARG, BAD_OP}
    finally:
        d.close()


def test_statuses_with_hash_collisions():
    """The test build's string hash keeps 4 bits (-DJANUS_TEST_HOOKS; tpset_dict.hpp's str_key, which tpset.hip's and
    keyspace.hip's inserts and update.hip's lookups share): a lookup that hashed differently from the inserts would find
    no key, and every probe chain is long.  In a child process through JANUS_GPU_LIB, as test_query_keys_gpu's."""
    lib = ROOT / "janus-crdt_amd" / "lib" / "libjanusgpu_test.so"
    assert lib.exists(), "the test build is made by __graft_entry__.build()"
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import janus_gpu as jg, test_update_keys_gpu as t\n"
            "assert 'libjanusgpu_test' in str(jg.LIB_PATH)\n"
            "ctx = jg.Context(0)\nt.collision_scenario(ctx)\nctx.close()\nprint('PARITY OK')\n"
            % (str(ROOT / "janus-crdt_amd"), str(ROOT / "tests")))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240, env=dict(os.environ, JANUS_GPU_LIB=str(lib)),
                         cwd=str(ROOT / "tests"))
    assert out.returncode == 0 and "PARITY OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


def test_state_that_changes_between_calls(ctx):
    d = Duo(ctx, rows=16, R=3, eb=8, seed=4)
    try:
        d.add_keys([b"p0", b"s0"], [0, 1], [0, 0])

        def probe():
            ks = list(d.a.guid) + [b"absent"]
            return d.run([(k, INC, 3) for k in ks] + [(k, ADD, b"e0") for k in ks])

        probe()
        # registrations after a call: the dirty slots are uploaded by the next one
        d.add_keys([b"p1", b"s1"], [0, 1], [5, 1])
        d.a.create([b"late"])
        assert probe()["status"][4] == NO_CRDT
        g = [d.a.guid[b"late"]]
        d.a.register(g, [0], [15]), d.b.register(g, [0], [15])
        assert probe()["status"][4] == OK
        # 3000 registrations: the uid table rehashes (a whole upload)
        for w in (d.a, d.b):
            w.pnc.reserve(4000, 0)
        z = np.zeros((4000 - 16, 3), np.int64)
        d.P, d.N = np.vstack([d.P, z]), np.vstack([d.N, z])
        d.add_keys([b"bulk-%d" % i for i in range(3000)], [0] * 3000, list(range(16, 3016)))
        probe()
        # keys learnt from a peer between calls (KeySpace.receive)
        gs = J.random_guids(d.rng, 40)
        new = [b"peer-%d" % i for i in range(40)]
        assert d.ks.receive([msg([entry(k, g) for k, g in zip(new[:20], gs[:20])]), msg([entry(k, g) for k, g in zip(new[20:], gs[20:])])]) == 40
        for k, g in zip(new, gs):
            d.a.guid[k] = g
        nk = len(d.a.guid)
        assert (probe()["status"][nk - 40:nk] == NO_CRDT).all()
        for w in (d.a, d.b):
            w.register(gs, [0, 1] * 20, [3100 + i for i in range(40)])
        probe()
        # jg_pnc_reserve, both dimensions: the adds go to row * R + col of the new shape
        for w in (d.a, d.b):
            w.pnc.reserve(5000, 6)
        assert d.a.pnc.shape()[:2] == (5000, 6)
        P, N = np.zeros((5000, 6), np.int64), np.zeros((5000, 6), np.int64)
        P[:4000, :3], N[:4000, :3] = d.P, d.N
        d.P, d.N = P, N
        d.add_keys([b"grown"], [0], [4999])
        d.run([(b"grown", INC, 11), (b"p0", DEC, 4), (b"bulk-2999", INC, 1)], col=5)
        # a batch large enough to rebuild the element table
        names = [b"name-%d" % i for i in range(6000)]
        d.run([((b"s0", b"s1")[i & 1], ADD, nm) for i, nm in enumerate(names)], compare_stores=False)
        d.run([((b"s0", b"s1")[i & 1], REMOVE, nm) for i, nm in enumerate(names[:300])] + [(b"s0", ADD, b"after the rebuild")])
    finally:
        d.close()


def test_the_dense_merge_shadow_is_dropped(ctx):
    """Three dense identity merges leave the int64 store's shadow valid; update_keys writes through rw_P / rw_N, so the
    next dense merge must not read a stale shadow."""
    d = Duo(ctx, rows=256, R=4, eb=8, orset=False, seed=6)
    try:
        d.add_keys([b"c-%d" % i for i in range(256)], [0] * 256, list(range(256)))
        small = np.random.default_rng(7).integers(0, 1000, (256, 4)).astype(np.int64)
        d.reset_cells(small, small // 2)
        for w in (d.a, d.b):
            for _ in range(3):
                w.pnc.merge_rows(small, small // 2)
        assert d.a.pnc.dense_filter_state() == 2
        d.run([(b"c-%d" % (i % 256), INC if i % 2 else DEC, 5000 + i) for i in range(700)], col=1)
        assert d.a.pnc.dense_filter_state() == 0
        B = small + 3000  # below some raised cells, above the others
        for w in (d.a, d.b):
            w.pnc.merge_rows(B, B)
        d.P, d.N = orc.pnc_merge(d.P, d.N, B, B)
        d.compare_stores()
    finally:
        d.close()


def test_refusals_leave_outputs_and_stores_untouched(ctx, duos):
    d = duos[8]
    lib, p = jg.load(), jg._ptr
    cmds = [(b"pn-0", INC, 5), (b"set-0", ADD, b"refused"), (b"set-1", ADD, NA), (b"nope", DEC, 1)]
    n = len(cmds)
    koff, kdata, op, flag, amount, eoff, edata = jg.pack_commands([c[0] for c in cmds], [c[1] for c in cmds], [c[2] for c in cmds])
    lo, hi = d.tags(n)
    OUT = ("status", "result", "kind", "idx", "elem", "guid", "add_lim", "rem_lim")

    def snapshot():
        return [x.copy() for x in d.a.pnc.read_rows()] + [x.copy() for x in d.a.ors.read()] + [d.a.ors.names_since(0)]

    def same(s1, s2):
        return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(s1, s2))

    def call(node=d.a.node._h, ks=d.ks._h, n=n, koff=koff, kdata=kdata, op=op, flag=flag, amount=amount, eoff=eoff, edata=edata, lo=lo, hi=hi,
             col=0, null=(), want=jg.JG_EINVAL, stores=True):
        out = {"status": np.full(4, 0xA5, np.uint8), "result": np.full(4, 0xA5, np.uint8), "kind": np.full(4, 0xA5, np.uint8),
               "idx": np.full(4, 0xA5A5A5A5, np.uint32), "elem": np.full(4, 0xA5A5A5A5, np.uint32), "guid": np.full(8, 0xA5A5A5A5A5A5A5A5, np.uint64),
               "add_lim": np.full(4, 0xA5A5A5A5A5A5A5A5, np.uint64), "rem_lim": np.full(4, 0xA5A5A5A5A5A5A5A5, np.uint64)}
        before, held = {k: v.copy() for k, v in out.items()}, snapshot() if stores else None
        rc = lib.jg_node_update_keys(node, ks, n, p(koff), p(kdata), p(op), p(flag), p(amount), p(eoff), p(edata), p(lo), p(hi), col,
                                     *(None if k in null else p(out[k]) for k in OUT))
        assert rc == want, (rc, want)
        if want != jg.JG_OK:
            for k in out:
                assert np.array_equal(out[k], before[k]), k
            assert not stores or same(snapshot(), held)
        return out

    for name in ("node", "ks", "op", "flag"):
        call(**{name: None})
    call(null=("status",))
    call(null=("result",))
    call(koff=None)
    call(koff=np.array([0, 4, 3, 9, 13], np.uint64))                  # offsets that decrease
    call(koff=np.array([1, 4, 9, 13, 17], np.uint64))                 # off[0] = 0 as everywhere else
    call(eoff=np.array([0, 0, 7, 3, 7], np.uint64))
    call(flag=np.array([3, 1, 4, 3], np.uint8))                       # an arg_flag above 3
    call(amount=None)                                                 # an integer without the amount array
    call(eoff=None)                                                   # a string without its arrays
    call(edata=None)
    call(lo=None)                                                     # an element without the tags
    call(hi=None)
    call(flag=np.array([3, 0, 2, 3], np.uint8), eoff=None, edata=None, lo=None)  # the null element needs them too
    call(col=4)                                                       # the store has 4 replica columns
    call(null=("add_lim",))
    call(null=("rem_lim",))
    call(n=(1 << 31) - 16)
    other = jg.Context(int(os.environ.get("JANUS_GPU_DEVICE", "0")))
    try:
        with jg.KeySpace(other, 8, 1 << 10) as ks2:                   # a key space and a node of different contexts
            call(ks=ks2._h)
    finally:
        other.close()
    # the OR-Set store held by an open wave, PN-Counter commands in the same batch: no row changes
    held = snapshot()  # (the stores are read outside the open waves)
    jg._check(lib.jg_orset_wave_begin(d.a.ors._h, 1, 16))
    try:
        call(stores=False)
    finally:
        jg._check(lib.jg_orset_wave_abort(d.a.ors._h))
    assert same(snapshot(), held)
    # a streamed node wave holds both stores; with a registration pending the call is refused for that as well
    assert lib.jg_apply_stream_begin(d.a.node._h, None, 10, 1 << 12) == jg.JG_OK
    try:
        call(stores=False)
        extra = d.a.create([b"registered-mid-stream"])
        d.a.register(extra, [0], [60])
        d.b.register(extra, [0], [60])
        call(stores=False)
    finally:
        at, nd = jg._u64(), jg._u64()
        assert lib.jg_apply_stream_end(d.a.node._h, None, C.byref(nd), C.byref(at)) == jg.JG_OK
    assert same(snapshot(), held)
    assert call(n=0, want=jg.JG_OK)["status"].tolist() == [0xA5] * 4
    # a PN-Counter-only batch may leave tags and elements NULL; the optional outputs are optional
    pn = jg.pack_commands([b"pn-0", b"pn-1", b"set-0", b"nope"], [INC, DEC, INC, INC], [1, 2, 3, 4])
    out = call(koff=pn[0], kdata=pn[1], op=pn[2], flag=pn[3], amount=pn[4], eoff=None, edata=None, lo=None, hi=None,
               null=("kind", "idx", "elem", "guid", "add_lim", "rem_lim"), want=jg.JG_OK)
    assert out["status"].tolist() == [OK, OK, BAD_ARG, NO_KEY] and out["result"].tolist() == [1, 1, 0, 0] and out["kind"].tolist() == [0xA5] * 4
    d.b.pnc.apply_ops([0, 1], [0, 0], [1, 2], [0, 1])
    d.P, d.N = orc.pnc_apply_ops(d.P, d.N, [0, 1], [0, 0], [1, 2], [0, 1])
    # and the first arguments, unbroken, apply
    d.run(cmds)


def test_writers_beside_a_reader(ctx):
    """Two threads write by key while a third reads by key on the same context: the calls are serialised by the context's
    lock, the adds commute, so the final values are the model's whatever the interleaving."""
    K = 128
    d = Duo(ctx, rows=K, R=4, eb=8, seed=9)
    try:
        zero = np.zeros((K, 4), np.int64)
        d.reset_cells(zero, zero)
        keys = [b"t-%d" % i for i in range(K)]
        d.add_keys(keys, [0] * K, list(range(K)))
        d.add_keys([b"t-set"], [1], [0])
        rng = np.random.default_rng(10)
        batches = {c: [[(keys[int(r)], INC if j % 3 else DEC, int(a)) for j, (r, a) in enumerate(zip(rng.integers(0, K, 300), rng.integers(-50, 1000, 300)))]
                       + [(b"t-set", ADD, b"by-%d-%d" % (c, b)), (b"missing", INC, 1)] for b in range(6)] for c in (0, 1)}
        errors = []

        def writer(col):
            try:
                for cmds in batches[col]:
                    got = d.a.node.update_keys(d.ks, [c[0] for c in cmds], [c[1] for c in cmds], [c[2] for c in cmds], tags=d.tags(len(cmds)), col=col)
                    if got["status"].tolist() != [OK] * 301 + [NO_KEY] or got["result"].tolist() != [1] * 301 + [0]:
                        errors.append("a writer's statuses")
            except Exception as e:  # noqa: BLE001
                errors.append(repr(e))

        def reader():
            try:
                for _ in range(20):
                    value, status, kind = d.a.node.query_keys(d.ks, keys + [b"missing"])
                    if not (status[:-1] == jg.JG_Q_OK).all() or status[-1] != jg.JG_Q_NO_KEY:
                        errors.append("a reader's statuses")
            except Exception as e:  # noqa: BLE001
                errors.append(repr(e))

        threads = [threading.Thread(target=writer, args=(0,)), threading.Thread(target=writer, args=(1,)), threading.Thread(target=reader)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=100)
        assert not any(t.is_alive() for t in threads), "a caller did not finish"
        assert not errors, errors
        P, N = d.P, d.N
        for col, bs in batches.items():
            for cmds in bs:
                pn = [c for c in cmds if c[0].startswith(b"t-") and c[0] != b"t-set"]
                P, N = orc.pnc_apply_ops(P, N, [int(c[0][2:]) for c in pn], [col] * len(pn), [c[2] for c in pn], [c[1] == DEC for c in pn])
        gP, gN = d.a.pnc.read_rows()
        assert np.array_equal(gP, P) and np.array_equal(gN, N)
        value, status, kind = d.a.node.query_keys(d.ks, keys)
        assert np.array_equal(value, orc.pnc_values(P, N)[0])
        assert sorted(d.a.ors.lookup_all_names([0])[0]) == sorted(b"by-%d-%d" % (c, b) for c in (0, 1) for b in range(6))
    finally:
        d.close()
