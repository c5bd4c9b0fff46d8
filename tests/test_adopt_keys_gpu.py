"""GPU: CRDT creation on the device (csrc/adopt.hip: jg_node_create_uids, jg_node_adopt_keys, jg_node_next_idx).

Every entry of every batch is compared, two ways: against tests/adopt_ref.py (the model of the allocation rule and the two
calls), and against a TWIN node built the old way — jg_node_register + jg_pnc_intern at the model's indices — through
jg_node_query_keys over every uid (each PN-Counter row holds row + 1, so a read names the row it reached),
jg_pnc_columns and jg_pnc_shape.  Uids aimed at one probe chain come from tests/node_hash.py.
"""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import adopt_ref as A
import janus_gpu as jg
import jsongen as J
import node_hash as H
import tpset_ref as TR

pytestmark = pytest.mark.gpu

CSRC = Path(__file__).resolve().parents[1] / "janus-crdt_amd" / "csrc"


def _const(file, name):
    m = re.search(r"constexpr uint32_t[^;]*\b%s = (\d+)" % name, (CSRC / file).read_text())
    assert m, name
    return int(m.group(1))


# the rank scans are jgt::excl_scan (block_scan.hpp): tiles of kBlock x kScanItems counts, one block up to four tiles
TILE = _const("tpset_dict.hpp", "kBlock") * _const("block_scan.hpp", "kScanItems")
R, EB = 2, 8
REP, OTHER = (0x5E1F, 0xA11CE), (0x0B0B, 0xB0B0)


def uids_of(rng, n):
    out = J.random_guids(rng, n)
    assert len(set(out)) == n
    return out


def split(uids):
    return [u[0] for u in uids], [u[1] for u in uids]


class Rig:
    """The node under test over its own stores, and its model."""

    def __init__(self, ctx, n_keys=4, orset=True):
        self.ctx = ctx
        self.pnc = jg.PNCStore(ctx, n_keys, R, EB) if n_keys else None
        self.orset = jg.ORSetStore(ctx) if orset else None
        self.node = jg.Node(self.pnc, self.orset)
        self.model = A.NodeModel(n_keys, R if n_keys else 0, orset)
        self.closers = [self.node, self.pnc, self.orset]

    def close(self):
        for c in self.closers:
            if c is not None:
                c.close()

    def state(self):
        return self.node.next_idx(), (self.pnc.shape() if self.pnc else None)

    def _both(self, lib, ref):
        """The call on the library and on the model: the same outputs, or the same refusal with nothing changed."""
        before = self.state()
        try:
            want = ref()
        except A.Refused as r:
            with pytest.raises(jg.JanusError) as e:
                lib()
            assert e.value.code == r.code and self.state() == before
            return None
        got = lib()
        for g, w in zip(got, want):
            assert np.array_equal(np.asarray(g, np.int64), np.asarray(w, np.int64))
        assert self.node.next_idx() == tuple(self.model.next)
        return got

    def register(self, uids, types, idx):
        return self._both(lambda: (self.node.register(*split(uids), types, idx), ())[1], lambda: (self.model.register(uids, types, idx), ())[1])

    def create(self, uids, types, replica=None, max_keys=0):
        return self._both(lambda: self.node.create_uids(*split(uids), types, replica, max_keys),
                          lambda: self.model.create_uids(uids, list(types), replica, max_keys))

    def adopt(self, pro, ks, from_, to, replica=None, max_keys=0):
        records = ks.new_keys(0)[0][from_:to]
        return self._both(lambda: self.node.adopt_keys(pro.node, ks, from_, to, replica, max_keys),
                          lambda: self.model.adopt(pro.model, records, replica, max_keys))

    def check(self, absent=()):
        """Every uid of the model, and some it lacks, read by name on the node and on a twin built with jg_node_register +
        jg_pnc_intern at the model's indices; the stores' shapes and replica tables."""
        m = self.model
        assert self.node.next_idx() == tuple(m.next)
        uids = list(m.uids) + list(absent)
        keys = [b"k%d" % i for i in range(len(uids))]
        tp = to = None
        ks = jg.KeySpace(self.ctx, len(uids) + 8, 64 * (len(uids) + 8))
        try:
            assert all(ks.create_keys(list(zip(keys, uids))))
            if self.pnc:
                assert self.pnc.shape() == (m.n_keys, R, EB)
                tp = jg.PNCStore(self.ctx, m.n_keys, R, EB)
            to = jg.ORSetStore(self.ctx) if self.orset else None
            twin = jg.Node(tp, to)
            try:
                if m.uids:
                    twin.register(*split(list(m.uids)), [k for k, _ in m.uids.values()], [i for _, i in m.uids.values()])
                for c in range(R):
                    rows = [r for r, cols in m.cols.items() if len(cols) > c]
                    if rows:
                        assert (tp.intern(rows, *split([m.cols[r][c] for r in rows])) == c).all()
                if self.pnc:
                    P = np.zeros((m.n_keys, R), np.int64)
                    P[:, 0] = np.arange(m.n_keys) + 1
                    self.pnc.write_rows(P, np.zeros_like(P))
                    tp.write_rows(P, np.zeros_like(P))
                    rows = np.arange(m.n_keys, dtype=np.uint32)
                    (g1, n1), (g2, n2) = self.pnc.columns(rows), tp.columns(rows)
                    assert np.array_equal(n1, n2) and np.array_equal(g1, g2)
                    assert n1.tolist() == [len(m.cols.get(r, ())) for r in range(m.n_keys)]
                got, want = self.node.query_keys(ks, keys), twin.query_keys(ks, keys)
                for a, b in zip(got, want):
                    assert np.array_equal(a, b)
                value, status, kind = got
                exp = [m.uids.get(u) for u in uids]
                assert kind.tolist() == [255 if e is None else e[0] for e in exp]
                assert status.tolist() == [jg.JG_Q_NO_CRDT if e is None else (jg.JG_Q_OK if e[0] == 0 else jg.JG_Q_NO_ARG) for e in exp]
                assert value.tolist() == [e[1] + 1 if e is not None and e[0] == 0 else 0 for e in exp]
            finally:
                twin.close()
        finally:
            for c in (tp, to, ks):
                if c is not None:
                    c.close()


@pytest.fixture
def rig(ctx):
    made = []

    def make(**kw):
        made.append(Rig(ctx, **kw))
        return made[-1]

    yield make
    for r in reversed(made):
        r.close()


def irregular_kinds(rng, n):
    """Runs of one kind of every length from 1 to a few hundred: the ranks of either kind cross wavefronts and workgroups."""
    out = []
    while len(out) < n:
        out += [len(out) % 2 if rng.integers(0, 2) else int(rng.integers(0, 2))] * int(rng.choice([1, 2, 3, 63, 64, 65, 255, 257, 300]))
    return out[:n]


@pytest.mark.parametrize("n", [0, 1, 65, 513, 3 * TILE + 1, 4 * TILE + 1])
def test_sizes(rig, n):
    """One call of n entries; 3 tiles + 1 ends a tile with one entry inside the one-block scan, 4 tiles + 1 is the first
    size the three-launch scan takes."""
    rng = np.random.default_rng(n)
    r = rig()
    r.create([(1, 1), (2, 2), (3, 3)], [1, 0, 1], replica=[OTHER] * 3)  # not from zero
    uids, kinds = uids_of(rng, n), irregular_kinds(rng, n)
    got = r.create(uids, kinds, replica=uids_of(rng, n), max_keys=1 << 16)
    assert got is not None and len(got[0]) == n
    r.check(absent=[(9, 9)])


def test_repeats_in_different_workgroups(rig):
    rng = np.random.default_rng(1)
    r = rig()
    uids, kinds = uids_of(rng, 2000), irregular_kinds(rng, 2000)
    for first, later in ((3, [1500]), (700, [701, 1999]), (0, [255, 256, 1024])):
        for j in later:
            uids[j], kinds[j] = uids[first], 1 - kinds[first]  # the repeat names the other type: the first stands
    status, idx = r.create(uids, kinds, replica=[REP] * 2000, max_keys=4096)
    assert status[[1500, 701, 1999, 255, 256, 1024]].tolist() == [jg.JG_C_EXISTS] * 6 and status.sum() == 6
    assert idx[1500] == idx[3] and idx[701] == idx[1999] == idx[700] and idx[255] == idx[256] == idx[1024] == idx[0]
    r.check()


def test_mixing_with_register(rig):
    r = rig(n_keys=16)
    a, b, c = (11, 1), (22, 2), (33, 3)
    r.register([a], [0], [7])
    assert r.node.next_idx() == (8, 0)  # one past the largest row, not the count
    status, idx = r.create([a, b, c], [0, 0, 1])
    assert status.tolist() == [jg.JG_C_EXISTS, jg.JG_C_CREATED, jg.JG_C_CREATED] and idx.tolist() == [7, 8, 0]
    assert r.register([b], [0], [3]) is None  # the reverse order: jg_node_register refuses a created uid
    assert r.register([c], [1], [5]) is None
    r.register([(44, 4)], [1], [9])
    status, idx = r.create([(55, 5)], [1])
    assert idx.tolist() == [10]
    r.check()


def test_probe_chain_that_wraps(rig):
    """240 uids homing to the table's last slot, some with a zero half (neither half can be the insert's CAS target): a
    third registered by hand first, the rest created in two calls, then all of them again."""
    his = [None if k % 40 == 0 else (0 if k % 40 == 1 else 1000 + k) for k in range(240)]
    uids = H.clustered_uids(0, his)
    r = rig(n_keys=256)
    r.register(uids[0::3], [0] * 80, list(range(80)))
    s1, _ = r.create(uids[1::3] + uids[0:30:3], [k % 2 for k in range(90)])
    assert s1.tolist() == [jg.JG_C_CREATED] * 80 + [jg.JG_C_EXISTS] * 10
    r.create(uids[2::3], [1] * 80, replica=[REP] * 80)
    status, idx = r.create(uids, [0] * 240)
    assert (status == jg.JG_C_EXISTS).all() and idx.tolist() == [r.model.uids[u][1] for u in uids]
    r.check(absent=H.clustered_uids(240, [5, None]))


def test_table_growth_inside_and_between_calls(rig):
    rng = np.random.default_rng(2)
    r = rig(n_keys=0)  # OR-Set keys only: the table is what grows
    uids = uids_of(rng, 70_600)
    r.create(uids[:600], [1] * 600)  # 1,024 slots -> 4,096 before the kernels run
    status, idx = r.create(uids[300:], [1] * 70_300)  # -> 524,288
    assert status[:300].all() and not status[300:].any() and idx.tolist() == list(range(300, 70_600))
    r.check(absent=[(7, 7)])


def test_store_growth_and_its_limit(rig):
    rng = np.random.default_rng(3)
    r = rig(n_keys=4)
    uids = uids_of(rng, 100)
    r.create(uids[:10], [0] * 10, replica=[REP] * 10, max_keys=64)
    assert r.pnc.shape() == (10, R, EB)  # max(10, 2 x 4)
    P, N = r.pnc.read_rows()
    assert not P.any() and not N.any()
    r.create(uids[10:11], [0], max_keys=64)
    assert r.pnc.shape() == (20, R, EB)
    assert r.create(uids[11:80], [0] * 69, max_keys=64) is None  # 11 + 69 > 64: JG_ESTATE, nothing changed (_both)
    assert r.create(uids[11:21], [0] * 10, max_keys=0) is None  # no room, and the store may not grow
    r.check(absent=uids[11:21])
    r.create(uids[11:20] + uids[11:20], [0] * 18)  # fits exactly: repeats take no row
    assert r.node.next_idx() == (20, 0)
    r.check()


def entry(key, g):
    return key + b"\0" + TR.guid_d(g)


def adoption_scene(rig, ctx):
    """A journal holding status 1 / 2 / 3 records, a guid the prospective copy lacks, one the stable copy holds, two keys
    naming one guid."""
    pro, stb = rig(n_keys=8), rig(n_keys=8)
    u = [(0x100 + k, 0x200 + k) for k in range(6)]
    pro.create(u[:3], [0, 1, 0], replica=[OTHER] * 3)
    stb.register([u[2]], [0], [5])
    ks = jg.KeySpace(ctx, 64, 1 << 12)
    msg = TR.encode_msg([entry(b"a", u[0]), b"nonul", entry(b"b", u[3]), entry(b"c", u[2]), entry(b"d", u[1]), entry(b"e", u[0]),
                         b"g\0" + TR.guid_d(u[4])[:-1] + b"x", None, entry(b"zero", (0, 0))], [])
    assert ks.receive([msg]) == 9
    assert [s for _, _, s in ks.new_keys(0)[0]] == [0, 1, 0, 0, 0, 0, 2, 3, 0]
    return pro, stb, ks, u


def test_adoption(rig, ctx):
    pro, stb, ks, u = adoption_scene(rig, ctx)
    try:
        status, kind, idx = stb.adopt(pro, ks, 0, 9, replica=[REP] * 9)
        assert status.tolist() == [jg.JG_A_ADOPTED, jg.JG_A_SKIPPED, jg.JG_A_NO_TYPE, jg.JG_A_HAVE, jg.JG_A_ADOPTED, jg.JG_A_HAVE, jg.JG_A_SKIPPED,
                                   jg.JG_A_SKIPPED, jg.JG_A_NO_TYPE]
        assert idx.tolist()[:6] == [6, 0xFFFFFFFF, 0xFFFFFFFF, 5, 0, 6] and kind.tolist()[:6] == [0, 255, 255, 0, 1, 0]
        # the key whose uid nobody created is in the dictionary, and reads by its name answer NO_CRDT
        assert stb.node.query_keys(ks, [b"b"])[1].tolist() == [jg.JG_Q_NO_CRDT]
        pro.create([u[3]], [1])
        status, kind, idx = stb.adopt(pro, ks, 0, 9)  # the same range again
        assert status.tolist()[:6] == [jg.JG_A_HAVE, jg.JG_A_SKIPPED, jg.JG_A_ADOPTED, jg.JG_A_HAVE, jg.JG_A_HAVE, jg.JG_A_HAVE]
        assert (kind[2], idx[2]) == (1, 1)
        assert stb.adopt(pro, ks, 2, 5)[0].tolist() == [jg.JG_A_HAVE] * 3  # a sub-range: outputs at j - from
        assert len(stb.adopt(pro, ks, 4, 4)[0]) == 0
        with pytest.raises(jg.JanusError) as e:
            stb.node.adopt_keys(pro.node, ks, 0, 10)  # past the journal
        assert e.value.code == jg.JG_EINVAL
        stb.check(absent=[u[4], u[5]])
        pro.check()  # only read
    finally:
        ks.close()


def test_wave_and_reads_by_name_after_adoption(rig, ctx):
    """A committed wave on the adopted uids, then "gs" by name: the model's values; column 0 of each adopted PN-Counter
    row is its replica, the wave's other replica column 1."""
    pro, stb, ks, u = adoption_scene(rig, ctx)
    try:
        reps = [(0x700 + j, 0x7) for j in range(9)]
        stb.adopt(pro, ks, 0, 9, replica=reps)
        row = stb.model.uids[u[0]][1]
        elem = ("x", [(1, 2)])
        msgs = [J.encode_pnc([OTHER, reps[0]], [9, 4], [2, 1]), J.encode_orset([elem], []), J.encode_pnc([reps[0]], [3], [5])]
        done, cut, rc = stb.node.apply_committed(None, *split([u[0], u[1], u[0]]), [1, 1, 1], [1, 2, 3], msgs)
        assert rc == jg.JG_OK and cut is None
        g, n = stb.pnc.columns([row])
        assert n.tolist() == [2] and (int(g[0, 0]["lo"]), int(g[0, 0]["hi"])) == reps[0] and (int(g[0, 1]["lo"]), int(g[0, 1]["hi"])) == OTHER
        value, status, kind = stb.node.query_keys(ks, [b"a", b"e", b"d", b"d", b"c", b"b"], [None, None, "x", "y", None, None])
        assert status.tolist() == [jg.JG_Q_OK] * 5 + [jg.JG_Q_NO_CRDT]
        assert value.tolist() == [(9 + 4) - (2 + 5), (9 + 4) - (2 + 5), 1, 0, 0, 0] and kind.tolist() == [0, 0, 1, 1, 0, 255]
    finally:
        ks.close()


def test_open_streamed_wave_refuses(rig, ctx):
    pro, stb, ks, u = adoption_scene(rig, ctx)
    try:
        lib = jg.load()
        assert lib.jg_apply_stream_begin(stb.node._h, None, 4, 256) == jg.JG_OK
        stb.model.wave_open = True
        try:
            assert stb.create([u[5]], [0]) is None  # JG_EINVAL, nothing changed
            assert stb.adopt(pro, ks, 0, 9) is None
        finally:
            at = C.c_uint64()
            assert lib.jg_apply_stream_end(stb.node._h, None, None, C.byref(at)) == jg.JG_OK
            stb.model.wave_open = False
        stb.check(absent=[u[0], u[5]])
        assert stb.adopt(pro, ks, 0, 9)[0].tolist()[0] == jg.JG_A_ADOPTED
    finally:
        ks.close()


def test_foreign_uid_turns_the_shard_shortcut_off(rig):
    """jg_node_set_shard(0, 2): a created uid of shard 1 disables the shortcut as jg_node_register does — a wave must
    still apply that key's state (with the shortcut on, the gather drops it from the uid alone)."""
    rng = np.random.default_rng(4)
    pool = uids_of(rng, 64)
    own = [x for x in pool if H.shard_of_uid(*x, 2) == 0][:2]
    foreign = [x for x in pool if H.shard_of_uid(*x, 2) == 1][:1]
    r = rig(n_keys=8)
    r.node.set_shard(0, 2)
    r.create(own, [0, 0], replica=[REP] * 2)
    wave = own + foreign
    msgs = [J.encode_pnc([REP], [5 + k], [k]) for k in range(3)]
    assert r.node.apply_committed(None, *split(wave), [1] * 3, [1, 2, 3], msgs)[1:] == (None, jg.JG_OK)
    assert r.pnc.values()[0].tolist()[:3] == [5, 5, 0]
    r.create(foreign, [0], replica=[REP])
    assert r.node.apply_committed(None, *split(wave), [1] * 3, [4, 5, 6], msgs)[1:] == (None, jg.JG_OK)
    assert r.pnc.values()[0].tolist()[:3] == [5, 5, 5]
    r.node.set_shard(0, 2)  # the rescan finds the created foreign uid too
    msgs = [J.encode_pnc([REP], [20], [2])] * 3  # max with (5 + k, k): 20 - 2 on every row
    assert r.node.apply_committed(None, *split(wave), [1] * 3, [7, 8, 9], msgs)[1:] == (None, jg.JG_OK)
    assert r.pnc.values()[0].tolist()[:3] == [18, 18, 18]
