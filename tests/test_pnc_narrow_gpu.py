"""The narrow form of a received PN-Counter batch (csrc/pnc_dense.hip, jg_rows): an int64 batch without key indices whose
every cell is ABSENT or in (INT32_MIN, INT32_MAX] is held as 4-byte codes, decided at jg_rows_upload (chunk by chunk) or
jg_synth_pnc_rows, and the dense merge reads it in that form.  The form a batch took is observed through jg_rows_form
(0 wide, 1 narrow) and switched with jg_rows_set_narrow; every merged result is numpy.maximum on the host, compared bit
for bit through read_rows.

G = the cells one workgroup of the filtered kernel takes of a narrow batch (kNarrowCells x kNarrowVecs x
kNarrowBlock), mirrored here as literals with the upload's chunk rule; test_constants_match_the_source (no GPU) reads
the constexpr lines: the shape's in csrc/pnc_dense_kernels.hpp, kNarrowChunkCap's beside the upload in
csrc/pnc_dense.hip.  A 128-B line of A is 16 cells."""
import re
from pathlib import Path

import numpy as np
import pytest

import janus_gpu as jg

NARROW_CELLS = 2       # kNarrowCells
NARROW_VECS = 2        # kNarrowVecs
NARROW_BLOCK = 256     # kNarrowBlock
CHUNK_CAP = 16777216   # kNarrowChunkCap
G = NARROW_CELLS * NARROW_VECS * NARROW_BLOCK
LINE = 16
WAVE = 64 * NARROW_CELLS

CSRC = Path(__file__).resolve().parent.parent / "janus-crdt_amd" / "csrc"
HOMES = {"kNarrowCells": "pnc_dense_kernels.hpp", "kNarrowVecs": "pnc_dense_kernels.hpp", "kNarrowBlock": "pnc_dense_kernels.hpp",
         "kNarrowChunkCap": "pnc_dense.hip"}

I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
EDGES = [I64_MIN, I32_MIN - 1, I32_MIN, I32_MIN + 1, -1, 0, 1, I32_MAX - 1, I32_MAX, 2 ** 31, 2 ** 40, I64_MAX]
FITTING = [v for v in EDGES if v == I64_MIN or I32_MIN < v <= I32_MAX]
NOT_FITTING = [I32_MAX + 1, I32_MIN, I32_MIN - 1, I64_MAX]
MODES = ("narrow", "off", "wide")  # narrowing on; set off; on, but one cell of the batch does not fit


def chunk_cells(n):
    """Cells per staged chunk of an upload of n cells (upload_narrow_array): two chunks fit the array's upper half
    behind the 16-B aligned end of the codes."""
    stage_at = (4 * n + 15) // 16 * 16
    return min(max(8 * n - stage_at, 0) // 16, CHUNK_CAP)


def test_constants_match_the_source():
    got = {}
    for name in ("kNarrowCells", "kNarrowVecs", "kNarrowBlock", "kNarrowChunkCap"):
        src = (CSRC / HOMES[name]).read_text()
        m = re.findall(r"^constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, src, re.M)
        assert len(m) == 1, f"{name}: expected one `constexpr <type> {name} = <literal>;` line in csrc/{HOMES[name]}"
        got[name] = int(m[0])
    assert got == {"kNarrowCells": NARROW_CELLS, "kNarrowVecs": NARROW_VECS, "kNarrowBlock": NARROW_BLOCK, "kNarrowChunkCap": CHUNK_CAP}


def test_small_shapes_cross_chunk_boundaries():
    """The shapes below upload in several chunks, most with a ragged last one (no GPU: the rule alone)."""
    for n in (G - 1, G, G + 1, 2 * G + 7, 345 * 3):
        c = chunk_cells(n)
        assert 0 < c and 4 <= -(-n // c) <= 5, (n, c)
    assert [n % chunk_cells(n) for n in (G - 1, G + 1, 2 * G + 7)] == [3, 5, 3]
    assert [chunk_cells(n) for n in (1, 2, 3, 4)] == [0, 0, 0, 1]  # below four cells nothing can be staged


def _cells(rng, n_keys, R):
    """Counters as the workload holds them: 30 % zero, the rest in [0, 2^31 - 100]."""
    a = rng.integers(0, 2 ** 31 - 99, (n_keys, R), dtype=np.int64)
    a[rng.random((n_keys, R)) < 0.3] = 0
    return a


def _received(rng, n_rows, R):
    """A received batch as the workload's: 30 % ABSENT, the rest in [0, 2^31 - 2]."""
    b = rng.integers(0, 2 ** 31 - 1, (n_rows, R), dtype=np.int64)
    b[rng.random((n_rows, R)) < 0.3] = I64_MIN
    return b


def _cells_of(ctx, rows):
    """The int64 cells a batch holds, through the dense merge into a store of INT64_MIN (max(INT64_MIN, b) == b);
    reads the batch in its form and leaves the form alone."""
    s = jg.PNCStore(ctx, rows.n_rows, rows.R, 8)
    try:
        lowest = np.full((rows.n_rows, rows.R), I64_MIN, np.int64)
        s.write_rows(lowest, lowest)
        s.merge_batch(rows)
        return s.read_rows()
    finally:
        s.close()


def _holds(ctx, rows, P, N, what=""):
    gP, gN = _cells_of(ctx, rows)
    assert np.array_equal(gP, P), ("P", what, np.argwhere(gP != P)[:8].tolist())
    assert np.array_equal(gN, N), ("N", what, np.argwhere(gN != N)[:8].tolist())


# ---- form -------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 1), (3, 1), (4, 1), (2 * G + 7, 1), (345, 3)], ids=lambda sh: "%dx%d" % sh)
def test_fitting_upload_is_narrow(ctx, shape):
    """ABSENT and both ends of the fitting range included; the batch holds the uploaded cells."""
    n, R = shape
    rng = np.random.default_rng(n + R)
    P, N = _received(rng, n, R), _received(rng, n, R)
    P.reshape(-1)[[0, -1]] = [I32_MAX, I64_MIN]
    N.reshape(-1)[[0, -1]] = [I32_MIN + 1, I32_MAX]
    b = jg.Rows(ctx, n, R, 8)
    try:
        assert b.form() == 0
        b.upload(P, N)
        assert b.form() == 1
        _holds(ctx, b, P, N)
        assert b.form() == 1
    finally:
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("side", ["P", "N"])
@pytest.mark.parametrize("value", NOT_FITTING, ids=["i32max+1", "i32min", "i32min-1", "i64max"])
def test_one_cell_that_does_not_fit_makes_it_wide(ctx, value, side):
    """The cell in the first chunk, a middle chunk, the ragged last chunk and as the last cell; the batch holds the
    uploaded cells either way, and the same buffers take a fitting batch narrow again."""
    n = 2 * G + 7
    c = chunk_cells(n)
    last_start = (n - 1) // c * c
    assert n - last_start < c and n - last_start >= 2 and c <= n // 2 < last_start
    rng = np.random.default_rng(3)
    P, N = _received(rng, n, 1), _received(rng, n, 1)
    b = jg.Rows(ctx, n, 1, 8)
    try:
        for at in (0, n // 2, last_start, n - 1):
            bad = [P.copy(), N.copy()]
            bad[side == "N"][at, 0] = value
            b.upload(*bad)
            assert b.form() == 0, at
            _holds(ctx, b, bad[0], bad[1], at)
            b.upload(P, N)
            assert b.form() == 1, at
        _holds(ctx, b, P, N)
    finally:
        b.close()


@pytest.mark.gpu
def test_keyed_and_int32_batches_are_wide(ctx):
    rng = np.random.default_rng(4)
    n, R = 300, 8
    P, N = _received(rng, n, R), _received(rng, n, R)
    b = jg.Rows(ctx, n, R, 8)
    b4 = jg.Rows(ctx, n, R, 4)
    try:
        b.upload(P, N, np.arange(n, dtype=np.uint32)[::-1].copy())
        assert b.form() == 0
        b.synth(7)  # the key indices are kept: wide
        assert b.form() == 0
        b.upload(P, N)
        assert b.form() == 1
        P4 = rng.integers(0, 1000, (n, R)).astype(np.int32)
        b4.upload(P4, P4)
        assert b4.form() == 0
        b4.synth(7)
        assert b4.form() == 0
    finally:
        b.close()
        b4.close()


@pytest.mark.gpu
def test_synth_takes_the_form_of_an_upload_of_its_cells(ctx):
    n, R = 2 * G // 8 + 3, 8
    b, off, up = jg.Rows(ctx, n, R, 8), jg.Rows(ctx, n, R, 8), jg.Rows(ctx, n, R, 8)
    try:
        off.set_narrow(False)
        off.synth(11, key0=5)
        assert off.form() == 0
        P, N = _cells_of(ctx, off)
        assert (P == I64_MIN).any() and P.max() < I32_MAX and ((P >= 0) | (P == I64_MIN)).all()
        b.synth(11, key0=5)
        up.upload(P, N)
        assert b.form() == up.form() == 1
        _holds(ctx, b, P, N, "synth, narrow")
        _holds(ctx, up, P, N, "upload of the same cells")
    finally:
        b.close(), off.close(), up.close()


@pytest.mark.gpu
def test_set_narrow_widens_and_holds(ctx):
    """Off on a narrow batch widens it now (several passes: the batch is past 2 x 256 cells) and keeps later uploads
    and synths wide; on again lets the next upload narrow."""
    n = 2 * G + 7
    rng = np.random.default_rng(8)
    P, N = _received(rng, n, 1), _received(rng, n, 1)
    b = jg.Rows(ctx, n, 1, 8)
    try:
        b.upload(P, N)
        assert b.form() == 1
        b.set_narrow(False)
        assert b.form() == 0
        _holds(ctx, b, P, N, "widened")
        b.upload(P, N)
        assert b.form() == 0
        b.synth(3)
        assert b.form() == 0
        b.set_narrow(True)
        assert b.form() == 0  # the form changes where a batch is born
        b.upload(P, N)
        assert b.form() == 1
        _holds(ctx, b, P, N, "narrow again")
    finally:
        b.close()


# ---- merges -----------------------------------------------------------------------------------------------------------

def _same(s, eP, eN, what=""):
    P, N = s.read_rows()
    assert np.array_equal(P, eP), ("P", what, np.argwhere(P != eP)[:8].tolist())
    assert np.array_equal(N, eN), ("N", what, np.argwhere(N != eN)[:8].tolist())


def _run(ctx, A, steps, mode, reserved):
    """The store A merged with every (name, BP, BN) of steps, each uploaded as Rows and merged with
    merge_batch(async_=True).  Cell `reserved` of every BP (flat index; the store's cell there is >= 0) is ABSENT,
    or INT32_MIN in mode "wide": it does not fit and loses all the same.  Returns the store's final rows."""
    n_keys, R = A[0].shape
    s = jg.PNCStore(ctx, n_keys, R, 8)
    rows = {}
    try:
        s.write_rows(*A)
        cur = [A[0].copy(), A[1].copy()]
        for name, BP, BN in steps:
            BP = BP.copy()
            BP.reshape(-1)[reserved] = I32_MIN if mode == "wide" else I64_MIN
            n = BP.shape[0]
            if n not in rows:
                rows[n] = jg.Rows(ctx, n, R, 8)
                if mode == "off":
                    rows[n].set_narrow(False)
            b = rows[n]
            b.upload(BP, BN)
            assert b.form() == (1 if mode == "narrow" else 0), (mode, name)
            s.merge_batch(b, async_=True)
            ctx.fence()
            cur[0][:n] = np.maximum(cur[0][:n], BP)
            cur[1][:n] = np.maximum(cur[1][:n], BN)
            _same(s, cur[0], cur[1], (mode, name))
        assert s.dense_filter_state() == 2, mode
        return cur
    finally:
        s.close()
        for b in rows.values():
            b.close()


def _all_modes(ctx, A, steps, reserved):
    ends = [_run(ctx, A, steps, mode, reserved) for mode in MODES]
    for e in ends[1:]:
        assert np.array_equal(e[0], ends[0][0]) and np.array_equal(e[1], ends[0][1])


def _with_absent(rng, b, p=0.1):
    b[rng.random(b.shape) < p] = I64_MIN
    return b


SHAPES = [(G - 1, 1), (G, 1), (G + 1, 1), (2 * G + 7, 1), (345, 3)]  # 345 x 3 = 1035 cells: odd, past one workgroup


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda sh: "%dx%d" % sh)
def test_merge_sequences(ctx, shape):
    """cold, build, filtered x 3, below, equal; then nothing raised, a raised cell on each side of every line boundary,
    every cell raised, each followed by a batch below the raised values: ABSENT cells throughout, raised cells at both
    ends and in the trailing cells.  The three modes end in the same store."""
    n_keys, R = shape
    rng = np.random.default_rng(n_keys * 31 + R)
    A = [_cells(rng, n_keys, R), _cells(rng, n_keys, R)]
    cur = [A[0].copy(), A[1].copy()]
    steps = []

    def step(name, masks, up):
        B = []
        for a, m in zip(cur, masks):
            b = _with_absent(rng, a - 1)
            b[m] = a[m] + up
            B.append(b)
        steps.append((name, B[0], B[1]))
        cur[0], cur[1] = np.maximum(cur[0], B[0]), np.maximum(cur[1], B[1])

    def some():
        out = []
        for a in cur:
            m = rng.random(a.shape) < 0.05
            m.reshape(-1)[[0, -1, -2, -3, -4]] = True
            out.append(m)
        return out

    none = [np.zeros((n_keys, R), bool)] * 2
    edge = np.zeros(n_keys * R, bool)
    for at in range(LINE, n_keys * R, LINE):
        edge[at - 1] = edge[at] = True
    edge = [edge.reshape(n_keys, R)] * 2
    every = [np.ones((n_keys, R), bool)] * 2
    for name in ("cold", "build", "filtered 0", "filtered 1", "filtered 2"):
        step(name, some(), 1)
    step("below", none, 0)
    steps.append(("equal", cur[0].copy(), cur[1].copy()))
    for name, masks in (("none", none), ("edges", edge), ("all", every)):
        step(name, masks, 10)
        step(name + ", below", masks, -4)  # below the raised values, above what those cells held before: nothing changes
    assert max(cur[0].max(), cur[1].max()) <= I32_MAX
    _all_modes(ctx, A, steps, reserved=1)


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1, 3])
def test_batch_shorter_than_the_store(ctx, R):
    """A short identity batch makes the shadow valid (the clamp pass covers the rows behind it); a batch over all keys
    then raises cells in those rows."""
    n_rows = (G + 37) // R
    n_keys = n_rows + (G + 5) // R
    rng = np.random.default_rng(77 + R)
    A = [_cells(rng, n_keys, R), _cells(rng, n_keys, R)]
    short = lambda k: (_with_absent(rng, A[0][:n_rows] + k), _with_absent(rng, A[1][:n_rows] + k))
    steps = [("short, cold",) + short(1), ("short, build",) + short(2), ("short, filtered",) + short(1)]
    BP, BN = _with_absent(rng, A[0] + 1), _with_absent(rng, A[1] + 1)
    BP[n_rows:, 0] = A[0][n_rows:, 0] + 5  # raised cells behind the short batch's rows, P and N
    BN[-1, :] = A[1][-1, :] + 7
    steps += [("all keys", BP, BN), ("all keys, again", BP, BN), ("all keys, every cell", A[0] + 9, A[1] + 9)]
    _all_modes(ctx, A, steps, reserved=1)


@pytest.mark.gpu
def test_escape_cells_under_a_narrow_batch(ctx):
    """Store cells at and beyond both clamp values against every fitting edge value, in lines that mix escapes, known
    cells and raised cells: through the unfiltered kernel, the build launch and the filtered kernel."""
    a = np.repeat(np.array(EDGES, np.int64), len(FITTING))
    b = np.tile(np.array(FITTING, np.int64), len(EDGES))
    pad = 2 * G + 9 - a.size  # past two workgroups, an odd total
    rng = np.random.default_rng(9)
    fill = rng.integers(0, 1000, pad).astype(np.int64)
    A = [np.concatenate([a, fill])[:, None], np.concatenate([fill, a[::-1]])[:, None]]
    BP = np.concatenate([b, fill + rng.integers(-1, 2, pad)])[:, None]
    BN = np.concatenate([fill + rng.integers(-1, 2, pad), b])[:, None]
    absent = np.full_like(BP, I64_MIN)
    full = lambda v: np.full_like(BP, v)
    steps = [("pairs, cold", BP, BN), ("pairs rolled, build", np.roll(BP, 5, 0), np.roll(BN, 7, 0)), ("pairs, filtered", BP, BN),
             ("absent", absent, absent), ("rolled", np.roll(BP, 21, 0), np.roll(BN, 33, 0)),
             ("lowest codes", full(I32_MIN + 1), full(I32_MIN + 1)), ("around INT32_MAX", full(I32_MAX - 1), full(I32_MAX)),
             ("INT32_MAX", full(I32_MAX), full(I32_MAX))]
    _all_modes(ctx, A, steps, reserved=a.size)  # the first fill cell of P


# ---- route ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_route_widens_a_narrow_batch(ctx):
    """jg_rows_route of a narrow identity batch returns what the same batch returns with narrowing off; the batch is
    wide afterwards and still merges."""
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(5)
    n, R, world = 3001, 3, 4
    P, N = _received(rng, n, R), _received(rng, n, R)
    got = {}
    for mode in ("narrow", "off"):
        b = jg.Rows(ctx, n, R, 8)
        s = jg.PNCStore(ctx, n, R, 8)
        try:
            if mode == "off":
                b.set_narrow(False)
            b.upload(P, N)
            assert b.form() == (1 if mode == "narrow" else 0)
            k = torch.zeros(n, dtype=torch.int32, device=dev)
            dP = torch.zeros((n, R), dtype=torch.int64, device=dev)
            dN = torch.zeros_like(dP)
            counts = b.route(world, k.data_ptr(), dP.data_ptr(), dN.data_ptr())
            assert b.form() == 0
            got[mode] = (counts, k.cpu().numpy(), dP.cpu().numpy(), dN.cpu().numpy())
            AP, AN = _cells(rng, n, R), _cells(rng, n, R)
            s.write_rows(AP, AN)
            s.merge_batch(b)
            _same(s, np.maximum(AP, P), np.maximum(AN, N), mode)
        finally:
            b.close()
            s.close()
    assert int(got["narrow"][0].sum()) == n
    assert np.array_equal(np.sort(got["narrow"][2].reshape(-1)), np.sort(P.reshape(-1)))
    for x, y in zip(got["narrow"], got["off"]):
        assert np.array_equal(x, y)
