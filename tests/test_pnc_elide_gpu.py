"""Store elision in the PN-Counter merges (k_merge_dense, k_merge_grouped): a 128-B line of A is written back only
if a cell of the batch raised it.  Bit-exact against the oracle on the FULL P and N read back, so a store that was
skipped but needed fails (the cell stays behind) and a store of anything but the maximum fails too.

The batches sit on the edges of the elision: nothing changes; one raised cell at the first / last index, on both
sides of a 128-B line boundary, in the last whole vector and in the tail cells; P only and N only (the two arrays
are elided separately); a sparse and a dense random share; the same batch twice."""
import functools

import numpy as np
import pytest

import janus_gpu as jg
import oracle_ref as orc
from gen import random_pnc

pytestmark = pytest.mark.gpu

# (n_keys, R): tail only / vectors + tail / nv no multiple of 8 (a partial line group in a partial wave) /
# several blocks with a partial last one / many blocks
DENSE_SHAPES = [(1, 1), (3, 5), (33, 7), (257, 64), (4097, 2)]


def _dt(eb):
    return np.int32 if eb == 4 else np.int64


@functools.lru_cache(maxsize=None)
def _dense_a(n_keys, R, eb):
    """The local state of a dense shape (shared by its cases, read-only): the width's whole range short of its
    maximum, so a cell can still be raised by one."""
    rng = np.random.default_rng(n_keys * 1009 + R * 31 + eb)
    info = np.iinfo(_dt(eb))
    AP = random_pnc(rng, n_keys, R, eb, absent=False, hi=info.max - 1)
    AN = random_pnc(rng, n_keys, R, eb, absent=False, hi=info.max - 1)
    AP.setflags(write=False)
    AN.setflags(write=False)
    return AP, AN


def _edge_cells(n_keys, R, eb):
    """Flat cell indices where one raised cell meets an edge of the kernel: the first and last cell, the last cell
    of the first 128-B line and the first of the next, the same across the first wave's and the first block's end,
    the last cell of the last whole 16-B vector (the last active lane's) and the first tail cell behind it."""
    total, per_vec, per_line = n_keys * R, 16 // eb, 128 // eb
    nv = total // per_vec
    cells = {0, total - 1, per_line - 1, per_line, 64 * per_vec - 1, 64 * per_vec, 256 * per_vec - 1, 256 * per_vec,
             nv * per_vec - 1, nv * per_vec}
    return sorted(c for c in cells if 0 <= c < total)


def _below(rng, A, p_absent=0.3):
    """Rows at or below A cell by cell, some cells ABSENT: a batch that raises nothing."""
    info = np.iinfo(A.dtype)
    B = np.minimum(A, random_pnc(rng, A.shape[0], A.shape[1], A.dtype.itemsize, absent=False))
    B[rng.random(A.shape) < p_absent] = info.min
    return B


def _raise(rng, A, p):
    """At or below A, except a share p of the cells at A + 1."""
    B = _below(rng, A)
    m = rng.random(A.shape) < p
    B[m] = A[m] + 1
    return B


def _dense_batches(n_keys, R, eb, kind):
    AP, AN = _dense_a(n_keys, R, eb)
    rng = np.random.default_rng(n_keys * 7 + R + eb)
    info = np.iinfo(_dt(eb))
    if kind == "equal":
        yield AP.copy(), AN.copy()
    elif kind == "absent":
        yield np.full_like(AP, info.min), np.full_like(AN, info.min)
    elif kind == "one_cell":
        for c in _edge_cells(n_keys, R, eb):
            for in_p, in_n in ((True, True), (False, True), (True, False)):
                BP, BN = AP.copy(), AN.copy()
                if in_p:
                    BP.flat[c] += 1
                if in_n:
                    BN.flat[c] += 1
                yield BP, BN
    elif kind == "random":
        for p in (0.01, 0.5):
            yield _raise(rng, AP, p), _raise(rng, AN, p)


@pytest.mark.parametrize("kind", ["equal", "absent", "one_cell", "random"])
@pytest.mark.parametrize("eb", [4, 8])
@pytest.mark.parametrize("n_keys,R", DENSE_SHAPES)
def test_dense_merge_rows(ctx, n_keys, R, eb, kind):
    AP, AN = _dense_a(n_keys, R, eb)
    s = jg.PNCStore(ctx, n_keys, R, eb)
    try:
        for BP, BN in _dense_batches(n_keys, R, eb, kind):
            s.write_rows(AP, AN)  # a fresh A for every batch
            s.merge_rows(BP, BN)
            P, N = s.read_rows()
            eP, eN = orc.pnc_merge(AP, AN, BP, BN)
            assert np.array_equal(P, eP) and np.array_equal(N, eN)
    finally:
        s.close()


@pytest.mark.parametrize("eb", [4, 8])
@pytest.mark.parametrize("n_keys,R", DENSE_SHAPES)
def test_dense_same_batch_twice(ctx, n_keys, R, eb):
    """The second merge of a batch is the case in which every store is elided: the state stays what the first left."""
    AP, AN = _dense_a(n_keys, R, eb)
    BP, BN = next(_dense_batches(n_keys, R, eb, "random"))
    eP, eN = orc.pnc_merge(AP, AN, BP, BN)
    s = jg.PNCStore(ctx, n_keys, R, eb)
    try:
        s.write_rows(AP, AN)
        s.merge_rows(BP, BN)
        P1, N1 = s.read_rows()
        s.merge_rows(BP, BN)
        P2, N2 = s.read_rows()
    finally:
        s.close()
    assert np.array_equal(P1, eP) and np.array_equal(N1, eN)
    assert np.array_equal(P2, eP) and np.array_equal(N2, eN)


@pytest.mark.parametrize("eb", [4, 8])
@pytest.mark.parametrize("n_keys,R", [(33, 7), (257, 64)])
def test_dense_merge_batch_device_rows(ctx, n_keys, R, eb):
    """The same kernel through Rows.upload + merge_batch (the benchmark's path): nothing changes, one cell in N
    only, half the cells, and the last batch once more."""
    AP, AN = _dense_a(n_keys, R, eb)
    rng = np.random.default_rng(n_keys + eb)
    one = AN.copy()
    one.flat[128 // eb] += 1
    batches = [(AP.copy(), AN.copy()), (AP.copy(), one), (_raise(rng, AP, 0.5), _raise(rng, AN, 0.5))]
    batches.append(batches[-1])
    s = jg.PNCStore(ctx, n_keys, R, eb)
    b = jg.Rows(ctx, n_keys, R, eb)
    eP, eN = AP, AN
    try:
        s.write_rows(AP, AN)
        for BP, BN in batches:
            b.upload(BP, BN)
            s.merge_batch(b, async_=True)
            ctx.fence()
            eP, eN = orc.pnc_merge(eP, eN, BP, BN)
            P, N = s.read_rows()
            assert np.array_equal(P, eP) and np.array_equal(N, eN)
    finally:
        s.close()
        b.close()


# ---- the grouped path: merge_rows with keys, rows of whole 16-B vectors and R >= 32 ----------------------------
GROUPED_KEYS = 2000


@functools.lru_cache(maxsize=None)
def _grouped_a(R, eb):
    rng = np.random.default_rng(R * 13 + eb)
    hi = 1 << (30 if eb == 4 else 60)  # room below for the rows "at or below" and above for the raise
    AP = random_pnc(rng, GROUPED_KEYS, R, eb, absent=False, lo=0, hi=hi)
    AN = random_pnc(rng, GROUPED_KEYS, R, eb, absent=False, lo=0, hi=hi)
    AP.setflags(write=False)
    AN.setflags(write=False)
    return AP, AN


def _grouped_keys(rng):
    """A batch's keys in a random order: key 11 once, key 12 twice, key 13 seven times, and 300 draws from the
    other keys (some of them repeated).  Returns (keys, {key: its rows' batch indices in batch order})."""
    keys = np.concatenate([[11], [12] * 2, [13] * 7, rng.integers(100, GROUPED_KEYS, 300)]).astype(np.uint32)
    keys = rng.permutation(keys)
    return keys, {k: np.nonzero(keys == k)[0] for k in (11, 12, 13)}


def _rows_below(rng, A, keys):
    return _below(rng, A[keys])


def _merge_and_check(s, AP, AN, BP, BN, keys):
    s.write_rows(AP, AN)
    s.merge_rows(BP, BN, keys)
    P, N = s.read_rows()
    eP, eN = orc.pnc_merge(AP, AN, BP, BN, keys)
    assert np.array_equal(P, eP) and np.array_equal(N, eN)
    return eP, eN


@pytest.mark.parametrize("eb", [4, 8])
@pytest.mark.parametrize("R", [32, 64, 130])
def test_grouped_nothing_changes(ctx, R, eb):
    AP, AN = _grouped_a(R, eb)
    rng = np.random.default_rng(R + eb)
    keys, _ = _grouped_keys(rng)
    s = jg.PNCStore(ctx, GROUPED_KEYS, R, eb)
    try:
        eP, eN = _merge_and_check(s, AP, AN, _rows_below(rng, AP, keys), _rows_below(rng, AN, keys), keys)
    finally:
        s.close()
    assert np.array_equal(eP, AP) and np.array_equal(eN, AN)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("eb", [4, 8])
@pytest.mark.parametrize("R", [32, 64, 130])
def test_grouped_one_raising_cell_per_key(ctx, R, eb, where):
    """Keys held 1, 2 and 7 times whose only raising cell sits in the key's first, middle or last row of the batch
    (the list head is whichever row linked last, so the three cover the head, an inner and the last-linked row),
    at the first or last column, in P and N or in N only; every other row of the batch is at or below A."""
    AP, AN = _grouped_a(R, eb)
    rng = np.random.default_rng(R * 3 + eb)
    keys, rows_of = _grouped_keys(rng)
    BP0, BN0 = _rows_below(rng, AP, keys), _rows_below(rng, AN, keys)
    s = jg.PNCStore(ctx, GROUPED_KEYS, R, eb)
    try:
        for col in (0, R - 1):
            for in_p in (True, False):
                BP, BN = BP0.copy(), BN0.copy()
                for k, rows in rows_of.items():
                    m = rows[{"first": 0, "middle": len(rows) // 2, "last": -1}[where]]
                    BN[m, col] = AN[k, col] + 1
                    if in_p:
                        BP[m, col] = AP[k, col] + 1
                eP, eN = _merge_and_check(s, AP, AN, BP, BN, keys)
                assert all(eN[k, col] == AN[k, col] + 1 for k in rows_of)  # the batch is what it claims to be
                assert np.array_equal(eP, AP) != in_p
    finally:
        s.close()


@pytest.mark.parametrize("eb", [4, 8])
@pytest.mark.parametrize("R", [32, 64, 130])
def test_grouped_two_batches_over_the_same_keys(ctx, R, eb):
    """Two random batches over one set of keys back to back, then the first again (nothing left to raise)."""
    AP, AN = _grouped_a(R, eb)
    rng = np.random.default_rng(R * 5 + eb)
    keys, _ = _grouped_keys(rng)
    hi = 1 << (30 if eb == 4 else 60)
    batches = [(random_pnc(rng, keys.size, R, eb, lo=0, hi=hi), random_pnc(rng, keys.size, R, eb, lo=0, hi=hi)) for _ in range(2)]
    batches.append(batches[0])
    s = jg.PNCStore(ctx, GROUPED_KEYS, R, eb)
    eP, eN = AP, AN
    try:
        s.write_rows(AP, AN)
        for BP, BN in batches:
            s.merge_rows(BP, BN, keys)
            eP, eN = orc.pnc_merge(eP, eN, BP, BN, keys)
            P, N = s.read_rows()
            assert np.array_equal(P, eP) and np.array_equal(N, eN)
    finally:
        s.close()
