"""GPU: the elastic PN-Counter store (jg_pnc_reserve, jg_pnc_shape, jg_pnc_set_max_replicas; csrc/pnc.hip
k_restride, csrc/json.hip finish_wave_elastic).

A grown store holds its old contents padded with zeros: every contents check compares read_rows / columns with the
numpy image of the store before the call, zero-padded to the new shape (the Guids against the old table, every new
slot all-zero).  Every path is then run on a grown store against the oracle (oracle_ref.pnc_apply_json & co. on the
padded dense image), and the opt-in widening against the oracle's Dictionary, which never runs out of columns."""
import ctypes as C

import numpy as np
import pytest

import janus_gpu as jg
import oracle_ref as orc
from jsongen import encode_pnc, random_guids

pytestmark = pytest.mark.gpu


def _dt(eb):
    return np.int32 if eb == 4 else np.int64


def _pattern(rng, n_keys, R, eb):
    """Seeded cells: random values of the whole width with MIN (= a received row's ABSENT), -1, MAX and 0 strewn in."""
    info = np.iinfo(_dt(eb))
    a = rng.integers(info.min, info.max, (n_keys, R), dtype=_dt(eb), endpoint=True)
    special = np.array([info.min, -1, info.max, 0], _dt(eb))
    pick = rng.random((n_keys, R)) < 0.2
    a[pick] = special[rng.integers(0, 4, int(pick.sum()))]
    a[0, 0], a[-1, -1] = info.min, -1
    return a


def _pad(a, n_keys, R):
    out = np.zeros((n_keys, R), a.dtype)
    out[: a.shape[0], : a.shape[1]] = a
    return out


def _fill_table(rng, s, n_keys, R):
    """Key k gets k % (R + 1) columns (none .. full rows) through intern; returns the dense (cols, ncols) image."""
    cols = np.zeros((n_keys, R), jg.GUID_DTYPE)
    ncols = (np.arange(n_keys) % (R + 1)).astype(np.uint32)
    keys = np.repeat(np.arange(n_keys, dtype=np.uint32), ncols)
    lo = rng.integers(1, 2**63, keys.size, dtype=np.uint64)
    hi = rng.integers(0, 2**63, keys.size, dtype=np.uint64)
    got = s.intern(keys, lo, hi)
    c = np.concatenate([np.arange(n) for n in ncols]).astype(np.uint32) if keys.size else np.zeros(0, np.uint32)
    assert np.array_equal(got, c)
    cols["lo"][keys, c], cols["hi"][keys, c] = lo, hi
    return cols, ncols


def _same_table(s, cols, ncols):
    g, n = s.columns(np.arange(cols.shape[0], dtype=np.uint32))
    assert g.shape == cols.shape
    assert np.array_equal(n, ncols), "column counts differ"
    assert np.array_equal(g, cols), "replica table differs (old Guids kept, every new slot all-zero)"


# (eb, keys, R) -> (keys', R'): the smallest shapes at which each path of the re-stride copy can go wrong
RESTRIDE = [
    (4, 7, 1, 7, 2), (8, 7, 1, 7, 2), (4, 7, 3, 7, 5), (8, 7, 3, 7, 5),      # cell path (R = 1, eb = 4 is a legal store)
    (8, 7, 2, 7, 4), (4, 7, 4, 7, 12),                                        # vector path
    (4, 7, 3, 7, 4), (4, 7, 4, 7, 5),                                         # one side a whole vector, the other not
    (8, 5, 64, 5, 65), (8, 5, 64, 5, 128), (4, 5, 64, 5, 128), (8, 5, 200, 5, 256),  # across a wavefront
    (8, 3, 3, 3, 3), (4, 3, 3, 1000, 3), (8, 5000, 3, 5003, 3),               # keys only: the stride stays
    (8, 5000, 3, 7001, 8), (4, 5000, 3, 7001, 8),                             # both: several workgroups and a tail
    (8, 5000, 40, 5001, 72),                                                  # vector path, several workgroups
    # more units than one pass of the grid covers (2^16 blocks x 256 = 16.8M): 16.9M cells, and as many of the
    # table's vectors, so both paths stride
    (4, 70000, 33, 70001, 241),
]


@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("eb,k0,r0,k1,r1", RESTRIDE)
def test_restride_contents(ctx, eb, k0, r0, k1, r1, table):
    rng = np.random.default_rng(1000 * eb + 7 * k0 + r0 + r1)
    s = jg.PNCStore(ctx, k0, r0, eb)
    P, N = _pattern(rng, k0, r0, eb), _pattern(rng, k0, r0, eb)
    s.write_rows(P, N)
    if table:
        cols, ncols = _fill_table(rng, s, k0, r0)
    s.reserve(k1, r1)
    assert s.shape() == (k1, r1, eb) and (s.n_keys, s.R) == (k1, r1)
    gP, gN = s.read_rows()
    assert gP.shape == (k1, r1)
    assert np.array_equal(gP, _pad(P, k1, r1)) and np.array_equal(gN, _pad(N, k1, r1)), "old cells kept, new cells zero"
    if table:
        _same_table(s, _pad(cols, k1, r1), np.concatenate([ncols, np.zeros(k1 - k0, np.uint32)]))
    else:  # no table yet: created at first use, at the new shape
        _same_table(s, np.zeros((k1, r1), jg.GUID_DTYPE), np.zeros(k1, np.uint32))
    s.close()


def test_noops_and_refusals(ctx):
    rng = np.random.default_rng(3)
    s = jg.PNCStore(ctx, 5, 6, 4)
    P, N = _pattern(rng, 5, 6, 4), _pattern(rng, 5, 6, 4)
    s.write_rows(P, N)
    cols, ncols = _fill_table(rng, s, 5, 6)

    def unchanged(shape=(5, 6)):
        assert s.shape() == shape + (4,)
        gP, gN = s.read_rows()
        assert np.array_equal(gP, _pad(P, *shape)) and np.array_equal(gN, _pad(N, *shape))
        _same_table(s, _pad(cols, *shape), np.concatenate([ncols, np.zeros(shape[0] - 5, np.uint32)]))

    for nk, r in ((5, 6), (0, 0), (4, 6), (5, 1), (1, 1)):  # same or smaller: JG_OK, nothing happens
        s.reserve(nk, r)
        unchanged()
    for nk, r in ((5, 257), (2**32, 6)):  # past the replica table's 256 columns; past the 32-bit key index
        with pytest.raises(jg.JanusError) as e:
            s.reserve(nk, r)
        assert e.value.code == jg.JG_EINVAL
        unchanged()
    s.reserve(5, 256)  # the table's bound itself is legal
    unchanged((5, 256))
    s.close()
    # without a replica table the columns are not bounded by it
    s = jg.PNCStore(ctx, 2, 3, 8)
    s.reserve(2, 300)
    assert s.shape() == (2, 300, 8)
    with pytest.raises(jg.JanusError) as e:  # ... until the table is wanted
        s.columns(np.array([0], np.uint32))
    assert e.value.code == jg.JG_EINVAL
    s.close()


class Img:
    """A GPU store and the oracle's dense image of the same state (as test_json_gpu.Pair), which grows with it."""

    def __init__(self, ctx, n_keys, R, eb, stable):
        self.s = jg.PNCStore(ctx, n_keys, R, eb)
        ga = np.array(stable, dtype=np.uint64).reshape(-1, 2)
        assert (self.s.intern(np.arange(n_keys, dtype=np.uint32), ga[:, 0], ga[:, 1]) == 0).all()
        self.P, self.N = np.zeros((n_keys, R), _dt(eb)), np.zeros((n_keys, R), _dt(eb))
        self.cols = np.zeros((n_keys, R), orc.GUID_DTYPE)
        self.cols["lo"][:, 0], self.cols["hi"][:, 0] = ga[:, 0], ga[:, 1]
        self.ncols = np.ones(n_keys, np.uint32)
        self.eb = eb

    def pad(self, n_keys, R):
        """The image padded to the store's new shape: what the store must hold after it grew."""
        self.ncols = np.concatenate([self.ncols, np.zeros(n_keys - self.P.shape[0], np.uint32)])
        self.P, self.N, self.cols = _pad(self.P, n_keys, R), _pad(self.N, n_keys, R), _pad(self.cols, n_keys, R)

    def follow(self):
        nk, r, _ = self.s.shape()
        self.pad(nk, r)

    def oracle(self, keys, msgs):
        self.P, self.N, self.cols, self.ncols, bad, rc = orc.pnc_apply_json(self.P, self.N, self.cols, self.ncols, keys, msgs, self.eb)
        return bad, rc

    def check(self):
        P, N = self.s.read_rows()
        assert np.array_equal(P, self.P) and np.array_equal(N, self.N), "values differ"
        _same_table(self.s, self.cols, self.ncols)

    def close(self):
        self.s.close()


def _capacity_wave(rng):
    """test_json_gpu.test_row_capacity_rolls_back's wave on a 3 x 3 store: key 2 would need 1 + 3 = 4 columns."""
    stable = random_guids(rng, 3)
    gs = random_guids(rng, 12)
    msgs = [encode_pnc(gs[:1], [1], [0]), encode_pnc(gs[:2], [2, 2], [0, 0]), encode_pnc([gs[0]], [3], [0]),
            encode_pnc(gs[:3], [1, 1, 1], [0, 0, 0])]
    return stable, gs, np.array([2, 1, 1, 2], np.uint32), msgs


@pytest.mark.parametrize("fuse", ["0", "1"])
@pytest.mark.parametrize("group", ["1", "8"])
def test_failed_wave_merges_after_reserve(ctx, group, fuse, monkeypatch):
    monkeypatch.setenv("JANUS_JSON_GROUP", group)
    monkeypatch.setenv("JANUS_JSON_FUSE", fuse)
    rng = np.random.default_rng(6)
    stable, gs, keys, msgs = _capacity_wave(rng)
    im = Img(ctx, 3, 3, 4, stable)
    with pytest.raises(jg.JanusError) as e:
        im.s.merge_json(keys, msgs)
    assert e.value.code == jg.JG_ESTATE and e.value.bad_msg == 3
    im.check()
    im.s.reserve(n_replicas=4)
    im.pad(3, 4)
    im.check()
    assert im.oracle(keys, msgs) == (None, 0)
    im.s.merge_json(keys, msgs)
    im.check()
    assert im.ncols.tolist() == [1, 3, 4]
    # steady waves over the new columns: every replica known, so a fused pass A applies them by itself
    for v in (7, 9):
        wave = [encode_pnc([stable[2]] + gs[:3], [v, v + 1, v + 2, v + 3], [1, 2, 3, v]), encode_pnc(gs[:2], [v + 5, 1], [v, v])]
        k = np.array([2, 1], np.uint32)
        assert im.oracle(k, wave) == (None, 0)
        im.s.merge_json(k, wave)
        im.check()
    im.close()


def test_values_apply_ops_and_encode_on_a_grown_store(ctx):
    rng = np.random.default_rng(12)
    MAX, MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min
    stable = random_guids(rng, 6)
    im = Img(ctx, 6, 64, 8, stable)
    im.P[0, 63], im.P[1, 63], im.P[2, 0], im.P[3, 10], im.N[4, 5], im.N[5, 63] = MAX - 5, MAX - 5, MAX, MAX, -1, 4
    im.s.write_rows(im.P, im.N)
    im.s.reserve(8, 128)
    im.pad(8, 128)
    # ops on new columns and on a new key; the checked sums' column order crosses the 64-column chunk
    key = np.array([0, 1, 1, 2, 3, 4, 5, 6, 7, 7], np.uint32)
    col = np.array([64, 64, 65, 64, 70, 100, 127, 0, 127, 64], np.uint32)
    delta = np.array([10, 10, -10, -1, 1, MIN, 9, 3, 5, 2], np.int64)
    is_n = np.array([0, 0, 0, 0, 0, 1, 1, 0, 1, 0], np.uint8)
    im.s.apply_ops(key, col, delta, is_n)
    im.P, im.N = orc.pnc_apply_ops(im.P, im.N, key, col, delta, is_n)
    im.check()
    v, o = im.s.values()
    ev, eo = orc.pnc_values(im.P, im.N)
    assert np.array_equal(v, ev) and np.array_equal(o, eo)
    assert eo.tolist() == [1, 1, 0, 1, 1, 0, 0, 0]  # key 1 overflows at column 64 although its whole sum fits
    # wire states naming replicas that land in the new columns, then Encode byte for byte (the cells zero again: the
    # ops above wrote columns no replica holds yet, which no Dictionary can)
    im.P[:], im.N[:] = 0, 0
    im.s.write_rows(im.P, im.N)
    gs = random_guids(rng, 80)
    msgs = [encode_pnc(gs, list(range(1, 81)), [0] * 80), encode_pnc(gs[70:] + gs[:3], [5] * 13, [6] * 13), encode_pnc(gs[:2], [1, 2], [3, 4])]
    k = np.array([5, 5, 7], np.uint32)
    assert im.oracle(k, msgs) == (None, 0)
    im.s.merge_json(k, msgs)
    im.check()
    assert im.ncols[5] == 81 and im.ncols[7] == 2 and im.ncols[6] == 0
    q = np.array([5, 0, 7], np.uint32)  # keys with a column (key 6 and 7 were born without the stable one)
    for kk, b in zip(q, im.s.encode_json(q)):
        c = int(im.ncols[kk])
        assert b == orc.json_encode_pnc(im.cols[kk, :c]["lo"], im.cols[kk, :c]["hi"], im.P[kk, :c], im.N[kk, :c], 8), f"key {kk}"
    im.close()


@pytest.mark.parametrize("eb", [4, 8])
def test_row_merges_on_a_grown_store(ctx, eb):
    """merge_rows / merge_batch with rows of the new shape and keys above the old n_keys: at R >= 32 the grouped
    merge runs, whose per-key heads were sized for the old key count by the merge before the store grew."""
    rng = np.random.default_rng(40 + eb)
    s = jg.PNCStore(ctx, 40, 32, eb)
    P, N = _pattern(rng, 40, 32, eb), _pattern(rng, 40, 32, eb)
    s.write_rows(P, N)
    keys = rng.integers(0, 40, 90).astype(np.uint32)
    BP, BN = _pattern(rng, 90, 32, eb), _pattern(rng, 90, 32, eb)
    s.merge_rows(BP, BN, keys)  # the heads exist now, for 40 keys
    P, N = orc.pnc_merge(P, N, BP, BN, keys)
    old = jg.Rows(ctx, 90, 32, eb)
    old.upload(BP, BN, keys)
    s.reserve(100, 64)
    P, N = _pad(P, 100, 64), _pad(N, 100, 64)
    keys = np.concatenate([rng.integers(0, 100, 300), [99, 99, 40, 40, 39]]).astype(np.uint32)
    BP, BN = _pattern(rng, keys.size, 64, eb), _pattern(rng, keys.size, 64, eb)
    s.merge_rows(BP, BN, keys)
    P, N = orc.pnc_merge(P, N, BP, BN, keys)
    gP, gN = s.read_rows()
    assert np.array_equal(gP, P) and np.array_equal(gN, N)
    keys = np.concatenate([rng.integers(0, 100, 200), [99, 41, 99]]).astype(np.uint32)
    BP, BN = _pattern(rng, keys.size, 64, eb), _pattern(rng, keys.size, 64, eb)
    new = jg.Rows(ctx, keys.size, 64, eb)
    new.upload(BP, BN, keys)
    s.merge_batch(new)
    P, N = orc.pnc_merge(P, N, BP, BN, keys)
    ident = jg.Rows(ctx, 100, 64, eb)  # an identity batch of the new shape: the dense merge
    IP, IN = _pattern(rng, 100, 64, eb), _pattern(rng, 100, 64, eb)
    ident.upload(IP, IN)
    s.merge_batch(ident, async_=True)
    s.reserve(101, 64)  # fences the async merge before the old buffers go
    P, N = orc.pnc_merge(P, N, IP, IN)
    P, N = _pad(P, 101, 64), _pad(N, 101, 64)
    gP, gN = s.read_rows()
    assert np.array_equal(gP, P) and np.array_equal(gN, N)
    with pytest.raises(jg.JanusError) as e:  # a batch created for the old R: the existing shape check's refusal
        s.merge_batch(old)
    assert e.value.code == jg.JG_ETYPE
    gP, gN = s.read_rows()
    assert np.array_equal(gP, P) and np.array_equal(gN, N)
    for r in (old, new, ident):
        r.close()
    s.close()


def test_open_wave_refuses_reserve(ctx):
    rng = np.random.default_rng(8)
    stable, gs, keys, msgs = _capacity_wave(rng)
    im = Img(ctx, 3, 3, 4, stable)
    im.s.wave_begin(4, 1024)
    im.s.wave_append(keys[:3], msgs[:3])
    with pytest.raises(jg.JanusError) as e:
        im.s.reserve(3, 4)
    assert e.value.code == jg.JG_EINVAL and im.s.shape() == (3, 3, 4)
    im.s.wave_abort()
    im.check()
    im.s.reserve(3, 4)
    im.pad(3, 4)
    im.check()
    assert im.oracle(keys, msgs) == (None, 0)
    im.s.merge_json(keys, msgs)
    im.check()
    im.close()


def _node(ctx, rng, im, n_keys):
    node = jg.Node(im.s, None)
    uids = random_guids(rng, n_keys)
    node.register([u[0] for u in uids], [u[1] for u in uids], [0] * n_keys, list(range(n_keys)))
    return node, uids


def test_open_node_stream_refuses_reserve(ctx):
    rng = np.random.default_rng(9)
    stable, gs, keys, msgs = _capacity_wave(rng)
    keys, msgs = keys[:3], msgs[:3]
    im = Img(ctx, 3, 3, 4, stable)
    node, uids = _node(ctx, rng, im, 3)
    lib = jg.load()
    assert lib.jg_apply_stream_begin(node._h, None, 3, sum(len(m) for m in msgs)) == jg.JG_OK
    c, keep = node._commit([uids[k][0] for k in keys], [uids[k][1] for k in keys], [1] * 3, [0] * 3, msgs)
    assert lib.jg_apply_stream_append(node._h, C.byref(c)) == jg.JG_OK
    with pytest.raises(jg.JanusError) as e:
        im.s.reserve(3, 4)
    assert e.value.code == jg.JG_EINVAL and im.s.shape() == (3, 3, 4)
    nd, at = C.c_uint64(), C.c_uint64()
    assert lib.jg_apply_stream_end(node._h, None, C.byref(nd), C.byref(at)) == jg.JG_OK and at.value == 2**64 - 1
    assert im.oracle(keys, msgs) == (None, 0)
    im.check()
    im.s.reserve(3, 4)  # the stream has ended: the store is the caller's again
    im.pad(3, 4)
    im.check()
    node.close()
    im.close()


# ---- the opt-in widening ---------------------------------------------------------------------------
def _merge(ctx, s, how, keys, msgs):
    if how == "json":
        s.merge_json(keys, msgs)
    elif how == "stream":
        s.wave_begin(len(msgs), 64)
        s.wave_append(keys[:1], msgs[:1])
        s.wave_append(keys[1:], msgs[1:])
        s.wave_commit()
    else:
        w = jg.Wave(ctx, len(msgs), sum(len(m) for m in msgs))
        w.upload(keys, msgs)
        try:
            s.merge_wave(w)
        finally:
            w.close()


@pytest.mark.parametrize("how", ["json", "stream", "wave"])
def test_auto_widening_merges_in_one_call(ctx, how):
    rng = np.random.default_rng(6)
    stable, gs, keys, msgs = _capacity_wave(rng)
    im = Img(ctx, 3, 3, 4, stable)
    im.s.set_max_replicas(8)
    _merge(ctx, im.s, how, keys, msgs)
    assert im.s.shape() == (3, 6, 4)
    im.pad(3, 6)
    assert im.oracle(keys, msgs) == (None, 0)
    im.check()
    # 3 -> 6 was one doubling; a key that then needs 7 columns takes the store to the bound itself
    msgs = [encode_pnc(gs[3:6], [4, 5, 6], [1, 1, 1]), encode_pnc(gs[:4], [9, 9, 9, 9], [0, 0, 0, 2])]
    keys = np.array([2, 0], np.uint32)
    _merge(ctx, im.s, how, keys, msgs)
    assert im.s.shape() == (3, 8, 4)
    im.pad(3, 8)
    assert im.oracle(keys, msgs) == (None, 0)
    im.check()
    assert im.ncols.tolist() == [5, 3, 7]
    im.close()


@pytest.mark.parametrize("how", ["json", "stream", "wave"])
@pytest.mark.parametrize("cap", [0, 3, 2])
def test_fixed_or_capped_store_fails_as_ever(ctx, cap, how):
    rng = np.random.default_rng(6)
    stable, gs, keys, msgs = _capacity_wave(rng)
    im = Img(ctx, 3, 3, 4, stable)
    if cap:
        im.s.set_max_replicas(cap)
    with pytest.raises(jg.JanusError) as e:
        _merge(ctx, im.s, how, keys, msgs)
    assert e.value.code == jg.JG_ESTATE and e.value.bad_msg == 3
    assert "more replicas than the store's columns" in str(e.value)
    assert im.s.shape() == (3, 3, 4)
    im.check()  # rolled back
    im.close()


def test_widening_stops_at_the_bound(ctx):
    rng = np.random.default_rng(16)
    stable, gs, keys, msgs = _capacity_wave(rng)
    im = Img(ctx, 3, 3, 4, stable)
    im.s.set_max_replicas(8)
    msgs = msgs + [encode_pnc(gs[:8], [1] * 8, [2] * 8)]  # key 1 would need 1 + 8 = 9 columns
    keys = np.append(keys, np.uint32(1))
    with pytest.raises(jg.JanusError) as e:
        im.s.merge_json(keys, msgs)
    assert e.value.code == jg.JG_ESTATE and e.value.bad_msg == 4
    im.follow()  # the contents before the call, padded to whatever the shape is now
    assert im.s.shape()[1] <= 8
    im.check()
    assert im.oracle(keys[:4], msgs[:4]) == (None, 0)  # the prefix the caller re-submits
    im.s.merge_json(keys[:4], msgs[:4])
    im.follow()
    im.check()
    im.close()


def test_intern_widens_and_stops_at_the_bound(ctx):
    s = jg.PNCStore(ctx, 4, 3, 8)
    s.set_max_replicas(8)
    keys = np.array([1, 0, 1, 1, 0, 1, 1], np.uint32)
    lo = np.array([10, 20, 11, 10, 21, 12, 13], np.uint64)
    assert s.intern(keys, lo, lo * 3).tolist() == [0, 0, 1, 0, 1, 2, 3]  # key 1's fourth replica: 3 -> 6 columns
    assert s.shape() == (4, 6, 8)
    g, n = s.columns(np.arange(4, dtype=np.uint32))
    assert n.tolist() == [2, 4, 0, 0] and g[1, :4]["lo"].tolist() == [10, 11, 12, 13] and not g[1, 4:]["lo"].any()
    with pytest.raises(jg.JanusError) as e:  # key 2 would need 9 columns under a bound of 8
        s.intern(np.array([3] + [2] * 9, np.uint32), np.arange(50, 60, dtype=np.uint64), np.arange(50, 60, dtype=np.uint64))
    assert e.value.code == jg.JG_ESTATE
    nk, r, _ = s.shape()
    assert r <= 8
    g2, n2 = s.columns(np.arange(4, dtype=np.uint32))
    assert n2.tolist() == [2, 4, 0, 0] and np.array_equal(g2, _pad(g, 4, r))  # all or nothing, padded
    s.close()


# ---- node waves --------------------------------------------------------------------------------------
def _node_wave(rng, uids):
    """40 states over 4 keys of a 4 x 3 store.  Keys hold their own replica and two more (full rows) until message
    25 names a third for key 1 (4 columns: the fixed store's cut), message 34 two more for key 2 (5) and message
    39 four more for key 3 (7: a second widening).  Every message is tracked."""
    per = [random_guids(rng, 6) for _ in range(4)]
    wave = []
    for i in range(40):
        k = i % 4
        gs = per[k][:2]
        if i == 25:
            gs = per[1][:3]
        elif i >= 33 and k == 2:
            gs = per[2][:4]
        elif i >= 37 and k == 3:
            gs = per[3][:6]
        if i > 25 and k == 1:
            gs = per[1][:3]
        wave.append((uids[k], k, i + 1, encode_pnc(gs, [i + 1 + c for c in range(len(gs))], [i // 3] * len(gs))))
    return wave


@pytest.mark.parametrize("mode", ["committed", "block", "stream"])
@pytest.mark.parametrize("cap", [0, 8])
def test_node_wave_cut_or_widened(ctx, cap, mode):
    rng = np.random.default_rng(77)
    im = Img(ctx, 4, 3, 4, random_guids(rng, 4))
    node, uids = _node(ctx, rng, im, 4)
    tr = jg.Tracker(ctx)
    wave = _node_wave(rng, uids)
    seqs = [w[2] for w in wave]
    tr.add(seqs, [1000 + q for q in seqs])
    if cap:
        im.s.set_max_replicas(cap)
    lo, hi, msgs = [w[0][0] for w in wave], [w[0][1] for w in wave], [w[3] for w in wave]
    if mode == "block":
        cut, rc = node.apply_block(lo, hi, [1] * 40, msgs)
        done = None
    elif mode == "stream":
        parts = [(lo[a:b], hi[a:b], [1] * (b - a), seqs[a:b], msgs[a:b]) for a, b in ((0, 11), (11, 30), (30, 40))]
        done, cut, rc = node.apply_stream(tr, parts)
    else:
        done, cut, rc = node.apply_committed(tr, lo, hi, [1] * 40, seqs, msgs)
    n = 40 if cap else 25
    if cap:
        assert (cut, rc) == (None, jg.JG_OK)
        assert im.s.shape() == (4, 8, 4)
        im.pad(4, 8)
    else:  # the fixed store: the wave is cut at the message whose key ran out of columns, its prefix applied
        assert (cut, rc) == (25, jg.JG_ESTATE)
        assert im.s.shape() == (4, 3, 4)
    assert im.oracle(np.array([w[1] for w in wave[:n]], np.uint32), msgs[:n]) == (None, 0)
    im.check()
    if done is not None:
        assert list(done) == [1000 + q for q in seqs[:n]]  # every completion, in commit order
        assert tr.size() == 40 - n
    tr.close()
    node.close()
    im.close()
