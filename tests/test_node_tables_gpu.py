"""The node's two open-addressing tables on the device (csrc/node.hip, csrc/uid_table.hpp) under the shapes the random
uids and identities of the other suites never make: probe chains hundreds of slots long that run off the table's last
slot to slot 0, tombstones in front of live entries, TryAdd after TryRemove, uids with a zero half, the uid table's
dirty-slot scatter and its growth between waves, pending tracker adds over several page-locked blocks, tracked identities
on messages the loop skips, and a tracker read while a streamed wave is open.

tests/node_hash.py inverts both table hashes (held to the C++ by tests/test_table_hash.py), so every cluster here is
aimed: a hash whose low 20 bits are ones homes to the last slot whatever capacity the library chose.  The tracker's
model is a Python dict in insertion order; the node's is test_node_gpu.Model (the oracle's loop); the reads and writes
by key name use the models of test_query_keys_gpu and test_update_keys_gpu.  Every check is exact.
"""
import ctypes as C

import numpy as np
import pytest

import janus_gpu as jg
import jsongen as J
import node_hash as H
import oracle_ref as orc
from orset_names_ref import ADD
from test_node_gpu import EB, Model, R, _setup
from test_query_keys_gpu import World
from test_update_keys_gpu import Duo

pytestmark = pytest.mark.gpu

MSG = J.encode_pnc([(1, 2)], [1], [0])
EMPTY_STATE = b'{"pVector":{},"nVector":{}}'


# ---- the tracker through a one-key PN-Counter node ---------------------------------------------------------------------
class OneKey:
    """A tracker, a node with one registered PN-Counter key, and the count of flushes: every size(), contains() and wave
    moves the pending adds to the device and switches the tracker's two page-locked buffers."""

    U = (0xABC, 0xDEF)

    def __init__(self, ctx):
        self.tr = jg.Tracker(ctx)
        self.pnc = jg.PNCStore(ctx, 4, R, EB)
        self.node = jg.Node(self.pnc, None)
        self.node.register([self.U[0]], [self.U[1]], [0], [0])
        self.flushes = 0

    def close(self):
        self.node.close()
        self.pnc.close()
        self.tr.close()

    def size(self):
        self.flushes += 1
        return self.tr.size()

    def contains(self, seqs):
        self.flushes += 1
        return self.tr.contains(seqs)

    def wave(self, seqs):
        """One committed wave of live states carrying `seqs`; the completed origins in commit order."""
        self.flushes += 1
        n = len(seqs)
        done, cut, rc = self.node.apply_committed(self.tr, [self.U[0]] * n, [self.U[1]] * n, [1] * n, seqs, [MSG] * n)
        assert cut is None and rc == jg.JG_OK
        return [int(o) for o in done]


def expect(model, seqs):
    """TryRemove in commit order: the first occurrence of a tracked identity reports its origin."""
    return [model.pop(s) for s in seqs if s in model]


def shuffled(rng, xs):
    xs = list(xs)
    return [xs[i] for i in rng.permutation(len(xs))]


@pytest.mark.parametrize("chunk", [None, 61])
def test_tracker_cluster_wraps_and_keeps_probing_past_tombstones(ctx, monkeypatch, chunk):
    """300 identities that all home to the LAST slot: the chain runs off the table's end to slot 0 and is 300 slots
    long.  TryAdd twice in one batch (first origin wins), ContainsKey of present and of never-added identities of the
    same home (the whole chain walked to its empty slot), completions in shuffled commit order, live entries found
    behind the tombstones those leave, TryAdd after TryRemove (a new entry with the new origin), TryAdd of a live
    identity (the old origin stays), and the chain emptied.  chunk 61: the claims on one identity come from
    different k_classify launches."""
    if chunk:
        monkeypatch.setenv("JANUS_WAVE_CHUNK", str(chunk))
        monkeypatch.setenv("JANUS_HOST_PAR_MIN", "1")
    rng = np.random.default_rng(3)
    k = OneKey(ctx)
    try:
        ids = H.clustered_seqs(0, 300)
        ghosts = H.clustered_seqs(300, 30)  # the same home, never added
        again = ids[7::15][:20]
        model = {s: 1000 + i for i, s in enumerate(ids)}
        k.tr.add(ids + again, [model[s] for s in ids] + [5000 + i for i in range(20)])  # one batch, distinct origins
        assert k.size() == 300
        assert k.contains(ids).all() and not k.contains(ghosts).any()
        # every third identity completes; some are committed twice, far apart, and ghosts ride along
        first = ids[::3]
        wave = shuffled(rng, first + first[::4] + ghosts[:10])
        assert k.wave(wave) == expect(model, wave)
        assert k.size() == len(model) == 200
        assert not k.contains(first).any() and k.contains(list(model)).all()  # live entries behind 100 tombstones
        assert not k.contains(ghosts).any()
        half = shuffled(rng, list(model)[::2])
        assert k.wave(half) == expect(model, half)
        assert k.size() == len(model) == 100
        # TryAdd after TryRemove: tracked again, with the new origin
        back = first[:50]
        k.tr.add(back, [9000 + i for i in range(50)])
        model.update({s: 9000 + i for i, s in enumerate(back)})
        assert k.size() == len(model) == 150 and k.contains(back).all()
        # TryAdd of live identities: false, the old origins stay
        live = [s for s in ids if s in model and s not in back][:50]
        k.tr.add(live, [7000 + i for i in range(50)])
        assert k.size() == 150
        wave = shuffled(rng, list(model) + live[:10] + ghosts[10:20])
        done = k.wave(wave)
        assert done == expect(model, wave) and len(done) == 150
        assert set(range(9000, 9050)) <= set(done) and not set(range(7000, 7050)) & set(done)
        assert k.size() == 0 and not model
        assert not k.contains(ids + ghosts).any()
    finally:
        k.close()


def test_tracker_rebuild_keeps_the_cluster(ctx):
    """The half-load rule rebuilds a 4,096-slot table (live + tombstones + pending > 2,048) into the spare: the 200
    survivors of a 300-identity cluster are re-slotted with their origins, the 100 completed stay absent, and size()
    equals the model after every step."""
    rng = np.random.default_rng(5)
    k = OneKey(ctx)
    try:
        ids = H.clustered_seqs(0, 300)
        ghosts = H.clustered_seqs(300, 30)
        model = {s: 1 + i for i, s in enumerate(ids)}
        k.tr.add(ids, list(model.values()))
        assert k.size() == 300
        gone = shuffled(rng, ids[1::3])
        assert k.wave(gone) == expect(model, gone)
        assert k.size() == len(model) == 200
        fresh = [int(x) for x in rng.integers(1, 2**63, 2500, dtype=np.uint64)]
        assert len(set(fresh) | set(ids)) == 2800
        for b in range(5):  # used = 300, 800, 1300, 1800: the fourth batch passes half of 4,096
            batch = fresh[500 * b:500 * (b + 1)]
            k.tr.add(batch, [100_000 + 500 * b + i for i in range(500)])
            model.update({s: 100_000 + 500 * b + i for i, s in enumerate(batch)})
            assert k.size() == len(model)
            assert not k.contains(gone).any() and not k.contains(ghosts).any()
        survivors = [s for s in ids if s in model]
        assert len(survivors) == 200 and k.contains(survivors).all() and k.contains(fresh).all()
        wave = shuffled(rng, survivors + gone[:20] + fresh[::5])
        done = k.wave(wave)
        assert done == expect(model, wave) and len(done) == 200 + 500
        assert k.size() == len(model) == 2000
        assert not k.contains(ids).any()
    finally:
        k.close()


def test_tracker_pending_adds_across_page_locked_blocks(ctx):
    """Pending adds fill a buffer's page-locked blocks of 65,536, 131,072, ... pairs in order.  Periods 1 and 2 put
    210,030 pairs (30 calls of 7,001: a call crosses each block boundary) into the first and the second buffer; period 3
    puts 70,000 into the first again, whose kept blocks are reused and whose third block stays empty.  An identity
    repeated across pair index 65,536 and across 196,608 keeps its first origin; completed identities of period 1 never
    come back (no stale pair of a reused block is replayed)."""
    rng = np.random.default_rng(7)
    k = OneKey(ctx)
    model, gone = {}, []
    try:
        for period, (n_calls, per, buffer) in enumerate([(30, 7001, 0), (30, 7001, 1), (10, 7000, 0)]):
            assert k.flushes % 2 == buffer  # which of the two buffers takes this period's adds
            n = n_calls * per
            seqs = np.arange(1, n + 1, dtype=np.uint64) + np.uint64(10_000_000 * (period + 1))
            orig = (np.arange(n) % 99991 + 1).astype(np.uint64)
            for a, b in ((65535, 65537), (65530, 65541), (196607, 196609), (196600, 196620)):
                if b < n:  # the same identity on either side of a block boundary, the later add with another origin
                    seqs[b], orig[b] = seqs[a], 2_000_000 + b
            for c in range(n_calls):
                k.tr.add(seqs[c * per:(c + 1) * per], orig[c * per:(c + 1) * per])
            for s, o in zip(seqs.tolist(), orig.tolist()):
                model.setdefault(s, o)
            assert k.size() == len(model)  # one flush of every block
            assert k.contains(seqs).all()
            at = set(np.linspace(0, n - 1, 3990).astype(np.int64).tolist()) | {0, 65535, 65536, 196607, 196608, n - 1}
            wave = shuffled(rng, [int(seqs[i]) for i in sorted(at) if i < n])
            done = k.wave(wave)
            assert done == expect(model, wave) and len(done) >= 3900
            gone += wave
            assert k.size() == len(model)
            assert not k.contains(wave).any()  # (five flushes a period: the next period's adds go to the other buffer)
        assert len(model) > 475_000 and not k.contains(gone).any()
    finally:
        k.close()


# ---- the node's model ----------------------------------------------------------------------------------------------
def _stores(ctx, rng, n_pnc):
    """test_node_gpu._setup without its registrations."""
    pnc = jg.PNCStore(ctx, n_pnc, R, EB)
    st = jg.ORSetStore(ctx)
    node = jg.Node(pnc, st)
    tr = jg.Tracker(ctx)
    m = Model(n_pnc, rng)
    pnc.intern(np.arange(n_pnc), [g[0] for g in m.own], [g[1] for g in m.own])
    return pnc, st, node, tr, m


def _check_wave(rng, pnc, st, node, tr, m, wave, how="call", block=False):
    """One wave through the library and through the model; everything test_node_gpu._run compares."""
    n_pnc = m.P.shape[0]
    exp_done, exp_cut = m.apply(wave, block=block)
    lo, hi = [x[0][0] for x in wave], [x[0][1] for x in wave]
    types, seqs, msgs = [x[1] for x in wave], [x[2] for x in wave], [x[3] for x in wave]
    if block:
        cut, rc = node.apply_block(lo, hi, types, msgs)
        done = []
    elif how == "stream":
        cuts = sorted(set(rng.integers(0, len(wave) + 1, 2).tolist()) | {0, len(wave)})
        parts = [(lo[a:b], hi[a:b], types[a:b], seqs[a:b], msgs[a:b]) for a, b in zip(cuts, cuts[1:])]
        done, cut, rc = node.apply_stream(tr, parts)
    else:
        done, cut, rc = node.apply_committed(tr, lo, hi, types, seqs, msgs)
    assert cut == exp_cut, (cut, exp_cut)
    assert (rc == jg.JG_OK) == (exp_cut is None)
    assert [int(o) for o in done] == exp_done
    P, N = pnc.read_rows()
    assert np.array_equal(P, m.P) and np.array_equal(N, m.N)
    g, nc = pnc.columns(np.arange(n_pnc))
    assert np.array_equal(nc, m.ncols)
    assert all(np.array_equal(g[k, :nc[k]], m.cols[k, :nc[k]]) for k in range(n_pnc))
    ga, gr = st.read()
    assert orc.same_orset(ga, gr, *m.orset)
    if not block:
        assert tr.size() == len(m.tracker)
        left = list(m.tracker)
        if left:
            assert tr.contains(left).all()
    assert node.stats()["msgs_applied"] == sum(1 for i, (u, t, _, _) in enumerate(wave)
                                               if t != 0 and u in m.keys and (exp_cut is None or i < exp_cut))
    st.names_sync()
    return [int(o) for o in done], cut, rc


class States:
    """Live states of registered keys: (uid, 1, identity, payload)."""

    def __init__(self, rng, m, n_pnc, n_set):
        self.rng, self.m = rng, m
        self.pcl = J.Cluster(rng, n_pnc, R - 1, EB, stable=None)
        self.ocl = J.ORSetCluster(rng, n_set)

    def of(self, uid, seq=0):
        t, idx = self.m.keys[uid]
        if t == 0:
            return (uid, 1, seq, self.pcl.message(idx))
        a, rr, na, nr = self.ocl.state(idx)
        return (uid, 1, seq, J.encode_orset(a, rr, na, nr))


def skipped(kind, uid, seq):
    """A message the loop skips, carrying an identity: a creation message, a key-space message, a state of an unknown
    uid."""
    if kind == 0:
        return (uid, 0, seq, b"junk: ManagerMsg_Create")
    if kind == 1:
        return ((0, 0), 1, seq, b"key space")
    return ((0x7777000000000000 + seq, 5), 1, seq, EMPTY_STATE)


@pytest.mark.parametrize("how", ["call", "stream"])
def test_identities_first_seen_on_skipped_messages(ctx, how):
    """A tracked identity whose first occurrence sits on a message the loop skips (ManagerMsg_Create, Guid.Empty, an
    unknown uid) takes no claim there: its later occurrence on a live state completes, at that message's commit
    position.  Before a cut, an identity seen only on a skipped message (its live occurrence after the cut) stays
    tracked and completes in the next wave."""
    rng = np.random.default_rng(11)
    n_pnc, n_set, n = 30, 8, 400
    pnc, st, node, tr, m, uids = _setup(ctx, rng, n_pnc, n_set)
    s = States(rng, m, n_pnc, n_set)
    seq = iter(range(1, 10**6))
    try:
        def base():
            return [s.of(uids[int(i)]) for i in rng.integers(0, len(uids), n)]

        def track(wave, at, origin):
            x = next(seq)
            wave[at] = wave[at][:2] + (x,) + wave[at][3:]
            m.tracker[x] = origin
            return x

        def fill(wave, taken):
            """Fresh tracked identities on two fifths of the other messages, some committed twice."""
            mine = []
            for i in range(n):
                if i not in taken and rng.random() < 0.4:
                    if mine and rng.random() < 0.1:
                        wave[i] = wave[i][:2] + (mine[int(rng.integers(0, len(mine)))],) + wave[i][3:]
                    else:
                        mine.append(track(wave, i, 50_000 + i))

        # wave 1: 30 identities first on a skipped message (10 of each kind), later on a live state
        wave = base()
        pos = sorted(rng.choice(n, 60, replace=False).tolist())
        special = {}
        for j in range(30):
            p1, p2 = pos[2 * j], pos[2 * j + 1]
            x = track(wave, p2, 1000 + j)
            wave[p1] = skipped(j % 3, uids[j], x)
            special[x] = 1000 + j
        fill(wave, set(pos))
        tr.add(list(m.tracker), list(m.tracker.values()))
        added = set(m.tracker)
        done, cut, rc = _check_wave(rng, pnc, st, node, tr, m, wave, how)
        assert cut is None and set(special.values()) <= set(done)
        live_at = {x[2]: i for i, x in reversed(list(enumerate(wave))) if x[1] != 0 and x[0] in m.keys}  # first live position
        order = [o for o in done if o in special.values()]
        assert order == [special[x] for x in sorted(special, key=live_at.get)]

        # wave 2: a rejected state at 200.  D: skipped before the cut, live after it.  E: skipped, then live, both before it.
        wave = base()
        c = 200
        before, after = sorted(rng.choice(c, 40, replace=False).tolist()), sorted((c + 1 + rng.choice(n - c - 1, 10, replace=False)).tolist())
        D, E = {}, {}
        for j in range(10):
            x = track(wave, after[j], 2000 + j)
            wave[before[j]] = skipped(j % 3, uids[j], x)
            D[x] = 2000 + j
        for j in range(15):
            p1, p2 = before[10 + 2 * j], before[11 + 2 * j]
            x = track(wave, p2, 3000 + j)
            wave[p1] = skipped(j % 3, uids[j], x)
            E[x] = 3000 + j
        fill(wave, set(before) | set(after) | {c})
        wave[c] = (uids[0], 1, wave[c][2], b'{"pVector":{}}')  # a PNCounterMsg Decode rejects (missing nVector)
        new = [x for x in m.tracker if x not in added]
        tr.add(new, [m.tracker[x] for x in new])
        added.update(new)
        done, cut, rc = _check_wave(rng, pnc, st, node, tr, m, wave, how)
        assert cut == c and rc != jg.JG_OK
        assert set(E.values()) <= set(done) and not set(D.values()) & set(done)
        assert tr.contains(list(D)).all() and not tr.contains(list(E)).any()

        # wave 3: D's identities on live states
        wave = base()
        for j, x in enumerate(shuffled(rng, D)):
            wave[7 * j + 3] = wave[7 * j + 3][:2] + (x,) + wave[7 * j + 3][3:]
        done, cut, rc = _check_wave(rng, pnc, st, node, tr, m, wave, how)
        assert cut is None and set(D.values()) <= set(done)
        assert not tr.contains(list(D)).any()
    finally:
        for h in (node, tr, pnc, st):
            h.close()


# ---- the uid table ------------------------------------------------------------------------------------------------------
def test_uid_cluster_upload_scatter_growth_and_block(ctx):
    """605 uids that all home to the LAST slot of the uid table (random hi halves, two with hi == 0, two with lo == 0),
    registered in four steps with a wave after each: 200 (the full upload), 100 more (dirty slots scattered into a chain
    that has wrapped past slot 0), 300 more (600 > 512: the host table rebuilt, the device table reallocated and
    uploaded whole), 5 more (a scatter into the grown table).  Each wave reaches every registered uid and carries 50
    states of never-registered uids of the same home, whose probes walk the whole chain: skipped, their tracked
    identities not completed.  Then a block with such a uid at index 137: jg_apply_block cuts there with JG_EINVAL after
    the 137 states before it."""
    rng = np.random.default_rng(41)
    total = 605
    types = [1 if i % 4 == 3 else 0 for i in range(total)]
    n_pnc, n_set = types.count(0), types.count(1)
    his = [int(x) for x in rng.integers(1, 2**64, total, dtype=np.uint64)]
    his[3], his[5], his[210], his[215] = 0, None, 0, None  # None: the uid whose lo is 0
    uids = H.clustered_uids(0, his)
    assert sum(1 for lo, hi in uids if lo == 0) == 2 and sum(1 for lo, hi in uids if hi == 0) == 2
    strangers = H.clustered_uids(5000, [int(x) for x in rng.integers(1, 2**64, 60, dtype=np.uint64)])
    idx, nxt = [], [0, 0]
    for t in types:
        idx.append(nxt[t])
        nxt[t] += 1
    pnc, st, node, tr, m = _stores(ctx, rng, n_pnc)
    s = States(rng, m, n_pnc, n_set)
    seq = iter(range(1, 10**6))
    try:
        reg = 0
        for count in (200, 100, 300, 5):
            node.register([u[0] for u in uids[reg:reg + count]], [u[1] for u in uids[reg:reg + count]], types[reg:reg + count], idx[reg:reg + count])
            for i in range(reg, reg + count):
                m.keys[uids[i]] = (types[i], idx[i])
            reg += count
            keys = list(range(reg)) + rng.integers(0, reg, 1450 - reg).tolist()
            wave, new = [], {}
            for i in keys:
                x = 0
                if rng.random() < 0.5:
                    x = next(seq)
                    new[x] = 1 + x % 9973
                wave.append(s.of(uids[i], x))
            lost = {}
            for u in strangers[:50]:
                x = next(seq)
                lost[x] = 20_000 + x
                wave.append((u, 1, x, EMPTY_STATE))
            wave = shuffled(rng, wave)
            m.tracker.update(new)
            m.tracker.update(lost)
            tr.add(list(new) + list(lost), list(new.values()) + list(lost.values()))
            done, cut, rc = _check_wave(rng, pnc, st, node, tr, m, wave)
            assert cut is None and len(done) == len(new)
            assert tr.contains(list(lost)).all()
        block = [s.of(uids[int(i)]) for i in rng.integers(0, total, 200)]
        block[137] = (strangers[55], 1, 0, EMPTY_STATE)
        done, cut, rc = _check_wave(rng, pnc, st, node, tr, m, block, block=True)
        assert cut == 137 and rc == jg.JG_EINVAL
    finally:
        for h in (node, tr, pnc, st):
            h.close()


def _named_cluster(rng):
    """64 key names whose Guids home to the last slot of the uid table (one with lo == 0, one with hi == 0), their types
    and indices, and a 65th name in the dictionary whose clustered Guid is never registered."""
    his = [None, 0] + [int(x) for x in rng.integers(1, 2**64, 63, dtype=np.uint64)]
    gs = H.clustered_uids(100, his)
    keys = [b"cl-%02d" % i for i in range(64)]
    types = [1 if i % 4 == 3 else 0 for i in range(64)]
    idx = [i % 3 if t else i for i, t in enumerate(types)]
    fill = [b"fill-%03d" % i for i in range(500)]
    return keys, gs, types, idx, b"cl-ghost", fill


def test_query_keys_through_a_uid_cluster(ctx):
    """jg_node_query_keys shares the probe (uid_find): 32 clustered keys registered before the first call (the full
    upload), 32 after it (the scatter), then 500 filler keys (564 > 512: growth).  Values and statuses equal the model and
    the composed path each time; the never-registered clustered Guid answers NO_CRDT after walking the chain."""
    rng = np.random.default_rng(51)
    keys, gs, types, idx, ghost, fill = _named_cluster(rng)
    w = World(ctx, rows=640, R=3, eb=8, seed=52)
    try:
        w.create(keys + [ghost], gs)
        w.ops([(sid, ADD, b"el-%d" % e) for sid in range(3) for e in range(sid + 1)])
        q = keys + [ghost, b"absent"]
        elems = [b"el-%d" % (i % 3) for i in range(len(q))]
        w.register(gs[:32], types[:32], idx[:32])
        value, status, kind, guid = w.check(q, elems)
        assert (status[:32] == jg.JG_Q_OK).all() and (status[32:65] == jg.JG_Q_NO_CRDT).all() and status[65] == jg.JG_Q_NO_KEY
        assert kind[:32].tolist() == types[:32] and value[3] == 1 and value[7] == 1  # sets 0 and 1 hold el-0 and el-1
        w.register(gs[32:64], types[32:], idx[32:])
        value, status, kind, guid = w.check(q, elems)
        assert (status[:64] == jg.JG_Q_OK).all() and status[64] == jg.JG_Q_NO_CRDT and kind[:64].tolist() == types
        w.add_keys(fill, [0] * 500, list(range(64, 564)))
        value, status, kind, guid = w.check(q + fill[::7], elems + [None] * len(fill[::7]))
        assert (status[:64] == jg.JG_Q_OK).all() and status[64] == jg.JG_Q_NO_CRDT and (status[66:] == jg.JG_Q_OK).all()
        w.check(q)  # no arguments: the OR-Set keys answer NO_ARG, still resolved through the cluster
    finally:
        w.close()


def test_update_keys_through_a_uid_cluster(ctx):
    """jg_node_update_keys over the same shapes: the commands of registered clustered keys apply (model and twin equal),
    those of the keys registered later answer NO_CRDT until they are, and the never-registered clustered Guid always."""
    rng = np.random.default_rng(53)
    keys, gs, types, idx, ghost, fill = _named_cluster(rng)
    d = Duo(ctx, rows=640, R=3, eb=8, seed=54)
    try:
        d.a.create(keys + [ghost], gs)
        cmds = [(k, ADD, b"e-%d" % (i % 5)) if t else (k, 1, 10 + i) for i, (k, t) in enumerate(zip(keys, types))]
        cmds += [(ghost, 1, 1), (b"absent", 1, 1)]
        OK, NO_KEY, NO_CRDT = jg.JG_U_OK, jg.JG_U_NO_KEY, jg.JG_U_NO_CRDT
        for w in (d.a, d.b):
            w.register(gs[:32], types[:32], idx[:32])
        got = d.run(cmds, col=1)
        assert (got["status"][:32] == OK).all() and (got["status"][32:65] == NO_CRDT).all() and got["status"][65] == NO_KEY
        assert got["idx"][:32].tolist() == idx[:32]
        for w in (d.a, d.b):
            w.register(gs[32:64], types[32:], idx[32:])
        got = d.run(cmds, col=2)
        assert (got["status"][:64] == OK).all() and got["status"][64] == NO_CRDT and got["idx"][:64].tolist() == idx
        d.add_keys(fill, [0] * 500, list(range(64, 564)))
        got = d.run(cmds + [(k, 2, 3) for k in fill[::7]], col=0)
        assert (got["status"][:64] == OK).all() and got["status"][64] == NO_CRDT and (got["status"][66:] == OK).all()
    finally:
        d.close()


# ---- a tracker read while a streamed wave is open --------------------------------------------------------------------
def test_tracker_read_while_a_streamed_wave_is_open(ctx):
    """Between jg_apply_stream_begin and _end the open wave classifies every part against the tracker table it began
    with and completes into it.  A jg_tracker_size in the middle, with 3,000 adds pending that no 4,096-slot table can
    take, must not move that table: the wave's completions are the model's for every identity added before begin, a
    late identity is reported or stays tracked (never both, never neither), size() and contains() agree with what was
    reported, and a following wave reports every leftover exactly once and nothing a second time."""
    rng = np.random.default_rng(61)
    n_pnc, n_set = 24, 6
    pnc, st, node, tr, m, uids = _setup(ctx, rng, n_pnc, n_set)
    s = States(rng, m, n_pnc, n_set)
    lib = jg.load()
    opened = False
    try:
        pre = H.clustered_seqs(0, 300) + [int(x) for x in rng.integers(1, 2**62, 300, dtype=np.uint64)]
        late = [int(x) for x in rng.integers(1, 2**62, 3000, dtype=np.uint64)]
        assert len(set(pre) | set(late)) == 3600
        origin = {x: 1 + i for i, x in enumerate(pre)}
        origin.update({x: 100_000 + i for i, x in enumerate(late)})
        pre_origins = {origin[x] for x in pre}
        tr.add(pre, [origin[x] for x in pre])                                   # 1. one batch, 300 of them a cluster

        def part(carried):
            ids = shuffled(rng, list(carried) + [0] * (300 - len(carried)))
            return [s.of(uids[int(k)], x) for k, x in zip(rng.integers(0, len(uids), 300), ids)]

        p1 = part(pre[:100] + pre[300:400])
        p2 = part(pre[100:200] + pre[400:500] + late[:100])
        both = p1 + p2

        def commit(p):
            return node._commit([x[0][0] for x in p], [x[0][1] for x in p], [x[1] for x in p], [x[2] for x in p], [x[3] for x in p])

        assert lib.jg_apply_stream_begin(node._h, tr._h, len(both), sum(len(x[3]) for x in both)) == jg.JG_OK  # 2. the first rebuild
        opened = True
        c1, keep1 = commit(p1)
        assert lib.jg_apply_stream_append(node._h, C.byref(c1)) == jg.JG_OK      # 3.
        tr.add(late, [origin[x] for x in late])                                 # 4. more than the table can take
        mid = tr.size()
        c2, keep2 = commit(p2)
        assert lib.jg_apply_stream_append(node._h, C.byref(c2)) == jg.JG_OK      # 5.
        at, nd = jg._u64(), jg._u64()
        out = np.zeros(len(both), np.uint64)
        rc = lib.jg_apply_stream_end(node._h, jg._ptr(out), C.byref(nd), C.byref(at))
        opened = False
        assert rc == jg.JG_OK and at.value == 2**64 - 1
        done = [int(o) for o in out[:nd.value]]

        m.tracker = {x: origin[x] for x in pre}
        exp_done, exp_cut = m.apply(both)
        assert exp_cut is None and len(exp_done) == 400
        size = tr.size()
        has = tr.contains(pre + late)
        reported = set(done)
        want = np.array([origin[x] not in reported for x in pre + late], np.uint8)
        print("mid-stream size %d (3600 added); %d reported; size after end %d (want %d); contains differs from added-and-not-reported at %d "
              "identities (%d reported ones still contained)"
              % (mid, len(done), size, 3600 - len(done), int((has != want).sum()), int(((has == 1) & (want == 0)).sum())))
        assert mid == 3600  # nothing completes before end
        assert [o for o in done if o in pre_origins] == exp_done  # every identity added before begin, in commit order
        late_done = [o for o in done if o not in pre_origins]
        assert len(set(done)) == len(done) and set(late_done) <= {origin[x] for x in late[:100]}
        assert size == 3600 - len(done)
        assert np.array_equal(has, want), "contains() != added and not reported"
        P, N = pnc.read_rows()
        assert np.array_equal(P, m.P) and np.array_equal(N, m.N)

        # every leftover identity, and 60 reported ones, in one wave: each leftover once, no origin a second time
        m.tracker = {x: origin[x] for x in pre + late if origin[x] not in reported}
        left = list(m.tracker)
        again = [x for x in pre + late if origin[x] in reported][::7][:60]
        carried = shuffled(rng, left + again)
        wave = [s.of(uids[int(k)], x) for k, x in zip(rng.integers(0, n_pnc, len(carried)), carried)]
        done2, cut, rc = _check_wave(rng, pnc, st, node, tr, m, wave)
        assert cut is None and sorted(done2) == sorted(origin[x] for x in left) and not set(done2) & reported
        assert tr.size() == 0 and not tr.contains(pre + late).any()
    finally:
        if opened:
            at, nd = jg._u64(), jg._u64()
            lib.jg_apply_stream_end(node._h, None, C.byref(nd), C.byref(at))
        for h in (node, tr, pnc, st):
            h.close()
