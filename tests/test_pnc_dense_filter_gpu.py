"""The dense PN-Counter merge by its 32-bit shadow (csrc/pnc_dense.hip pnc_merge_dense, csrc/pnc_dense_kernels.hpp): an
int64 store whose last writes were dense identity merges builds sP / sN = clamp32(P / N) at the second such merge
and reads them instead of P / N from the third on.  Every expected result is numpy.maximum on the host (or the
lowering the test applied), compared bit for bit through read_rows; the path a call took is observed through
jg_pnc_dense_filter_state (0 off or cold, 1 armed, 2 valid).

G = the cells one workgroup of the filtered kernel takes (kFiltCells x kFiltVecs x kFiltBlock), mirrored here as
literals; test_constants_match_the_kernel (no GPU) reads the kernel's constexpr lines.  A 128-B line of A is 16
cells, a wave-instruction covers 64 x kFiltCells cells."""
import re
from pathlib import Path

import numpy as np
import pytest

import janus_gpu as jg
from jsongen import encode_pnc, random_guids

FILT_CELLS = 2    # kFiltCells
FILT_VECS = 1     # kFiltVecs
FILT_BLOCK = 512  # kFiltBlock
G = FILT_CELLS * FILT_VECS * FILT_BLOCK
LINE = 16
WAVE = 64 * FILT_CELLS

KERNELS_HPP = Path(__file__).resolve().parent.parent / "janus-crdt_amd" / "csrc" / "pnc_dense_kernels.hpp"

I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
EDGES = [I64_MIN, I32_MIN - 1, I32_MIN, I32_MIN + 1, -1, 0, 1, I32_MAX - 1, I32_MAX, 2 ** 31, 2 ** 40, I64_MAX]


def test_constants_match_the_kernel():
    src = KERNELS_HPP.read_text()
    got = {}
    for name in ("kFiltCells", "kFiltVecs", "kFiltBlock"):
        m = re.findall(r"^constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, src, re.M)
        assert len(m) == 1, f"{name}: expected one `constexpr <type> {name} = <literal>;` line in csrc/pnc_dense_kernels.hpp"
        got[name] = int(m[0])
    assert got == {"kFiltCells": FILT_CELLS, "kFiltVecs": FILT_VECS, "kFiltBlock": FILT_BLOCK}


def _cells(rng, n_keys, R):
    """Counters as the workload holds them: 30 % zero, the rest anywhere in [0, 2^31 - 2]."""
    a = rng.integers(0, 2 ** 31 - 1, (n_keys, R), dtype=np.int64)
    a[rng.random((n_keys, R)) < 0.3] = 0
    return a


def _make_valid(s, AP, AN):
    """A = (AP, AN) with an exact shadow: two dense identity merges behind the write."""
    s.write_rows(AP, AN)
    assert s.dense_filter_state() == 0
    s.merge_rows(AP, AN)
    assert s.dense_filter_state() == 1
    s.merge_rows(AP, AN)
    assert s.dense_filter_state() == 2


def _same(s, eP, eN, what=""):
    P, N = s.read_rows()
    assert np.array_equal(P, eP), ("P", what, np.argwhere(P != eP)[:8].tolist())
    assert np.array_equal(N, eN), ("N", what, np.argwhere(N != eN)[:8].tolist())


def _merge(s, cur, BP, BN, what="", valid=True):
    """One dense merge of (BP, BN) into the store holding cur = [P, N]; cur becomes the host's numpy.maximum."""
    s.merge_rows(BP, BN)
    n = BP.shape[0]
    cur[0][:n] = np.maximum(cur[0][:n], BP)
    cur[1][:n] = np.maximum(cur[1][:n], BN)
    _same(s, cur[0], cur[1], what)
    if valid:
        assert s.dense_filter_state() == 2, what


# ---- state ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_states_cold_armed_valid(ctx):
    """cold -> armed -> valid over three identity merges (merge_batch, the benchmark's call, and merge_rows); a
    4-byte store stays at 0; with the filter set off the state stays 0 and the results are the same."""
    rng = np.random.default_rng(1)
    n_keys, R = 2 * G // 8 + 3, 8
    AP, AN = _cells(rng, n_keys, R), _cells(rng, n_keys, R)
    batches = [(_cells(rng, n_keys, R), _cells(rng, n_keys, R)) for _ in range(4)]
    results = {}
    for mode in ("on", "off", "rows"):
        s = jg.PNCStore(ctx, n_keys, R, 8)
        b = jg.Rows(ctx, n_keys, R, 8)
        try:
            if mode == "off":
                s.set_dense_filter(False)
            s.write_rows(AP, AN)
            cur = [AP.copy(), AN.copy()]
            seen = [s.dense_filter_state()]
            for BP, BN in batches:
                if mode == "rows":
                    s.merge_rows(BP, BN)
                else:
                    b.upload(BP, BN)
                    s.merge_batch(b, async_=True)
                    ctx.fence()
                seen.append(s.dense_filter_state())
                cur = [np.maximum(cur[0], BP), np.maximum(cur[1], BN)]
                _same(s, cur[0], cur[1], (mode, len(seen)))
            assert seen == ([0, 0, 0, 0, 0] if mode == "off" else [0, 1, 2, 2, 2]), (mode, seen)
            results[mode] = s.read_rows()
            if mode == "on":  # off drops a valid shadow, on again starts over from cold
                s.set_dense_filter(False)
                assert s.dense_filter_state() == 0
                s.set_dense_filter(True)
                s.merge_rows(*batches[0])
                assert s.dense_filter_state() == 1
                _same(s, cur[0], cur[1], "after off / on")
        finally:
            s.close()
            b.close()
    for mode in ("off", "rows"):
        assert np.array_equal(results[mode][0], results["on"][0]) and np.array_equal(results[mode][1], results["on"][1])
    s = jg.PNCStore(ctx, 64, 8, 4)
    try:
        A4 = rng.integers(0, 1000, (64, 8)).astype(np.int32)
        s.write_rows(A4, A4)
        for k in range(3):
            s.merge_rows(A4 + k, A4 + k)
            assert s.dense_filter_state() == 0
        P, N = s.read_rows()
        assert np.array_equal(P, A4 + 2) and np.array_equal(N, A4 + 2)
    finally:
        s.close()


# ---- the store's file and the dense merge's file meet -----------------------------------------------------------------

def _tiny_valid(ctx, rng):
    """An int64 store of 3 keys x 5 replicas (15 cells: a trailing cell, less than one workgroup) made valid by three
    jg_pnc_merge_batch calls; returns the store and the host's [P, N]."""
    n_keys, R = 3, 5
    cur = [_cells(rng, n_keys, R), _cells(rng, n_keys, R)]
    s = jg.PNCStore(ctx, n_keys, R, 8)
    b = jg.Rows(ctx, n_keys, R, 8)
    try:
        s.write_rows(cur[0], cur[1])
        for want in (1, 2, 2):
            BP, BN = _cells(rng, n_keys, R), _cells(rng, n_keys, R)
            b.upload(BP, BN)
            s.merge_batch(b)
            cur = [np.maximum(cur[0], BP), np.maximum(cur[1], BN)]
            assert s.dense_filter_state() == want
        _same(s, cur[0], cur[1], "tiny, valid")
    except BaseException:
        s.close()
        raise
    finally:
        b.close()
    return s, cur


@pytest.mark.gpu
def test_reserve_between_batch_merges(ctx):
    """jg_pnc_reserve (the store's file) drops a shadow that jg_pnc_merge_batch (the dense merge's file) built: the
    state reads cold at 4 x 6, and the next batch merges by the cells, not by a shadow of the old shape."""
    rng = np.random.default_rng(31)
    s, cur = _tiny_valid(ctx, rng)
    b = jg.Rows(ctx, 4, 6, 8)
    try:
        s.reserve(4, 6)
        assert s.dense_filter_state() == 0
        grown = []
        for c in cur:
            g = np.zeros((4, 6), np.int64)
            g[:3, :5] = c
            grown.append(g)
        BP, BN = _cells(rng, 4, 6), _cells(rng, 4, 6)
        b.upload(BP, BN)
        s.merge_batch(b)
        eP, eN = np.maximum(grown[0], BP), np.maximum(grown[1], BN)
        assert s.dense_filter_state() == 1
        _same(s, eP, eN, "after reserve")
        v, o = s.values()
        assert np.array_equal(v, eP.sum(1) - eN.sum(1)) and not o.any()
    finally:
        b.close()
        s.close()


@pytest.mark.gpu
def test_merge_rows_into_a_valid_store(ctx):
    """jg_pnc_merge_rows without key indices (the store's file, staged through scratch) reaches the filtered kernel
    through jg::pnc_merge_dense: one cell at INT32_MAX + 1 and one at INT32_MIN, and the state stays valid."""
    rng = np.random.default_rng(32)
    s, cur = _tiny_valid(ctx, rng)
    try:
        BP, BN = cur[0] - 1, cur[1] - 1
        BP[1, 2] = I32_MAX + 1
        BN[2, 4] = I32_MIN  # the trailing cell
        _merge(s, cur, BP, BN, "escape values")
        assert cur[0][1, 2] == I32_MAX + 1
        _merge(s, cur, BP, BN, "again")
    finally:
        s.close()


# ---- shape edges ------------------------------------------------------------------------------------------------------

SHAPES = [(G - 1, 1), (G, 1), (G + 1, 1), (2 * G + 7, 1), (345, 3)]  # 345 x 3 = 1035 cells: odd, past one workgroup


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda sh: "%dx%d" % sh)
def test_shape_edges(ctx, shape):
    """Store sizes around one workgroup's cells and a cell count that is no multiple of 4: raised cells at random,
    at both ends and in the trailing cells, through the build launch (second merge) and the filtered kernel."""
    n_keys, R = shape
    rng = np.random.default_rng(n_keys * 31 + R)
    AP, AN = _cells(rng, n_keys, R), _cells(rng, n_keys, R)
    AP, AN = np.minimum(AP, 2 ** 31 - 100), np.minimum(AN, 2 ** 31 - 100)

    def raised(cur, p):
        out = []
        for a in cur:
            b = a - 1
            m = rng.random(a.shape) < p
            m.reshape(-1)[[0, -1, -2, -3, -4]] = True
            b[m] = a[m] + 1
            out.append(b)
        return out

    s = jg.PNCStore(ctx, n_keys, R, 8)
    try:
        s.write_rows(AP, AN)
        cur = [AP.copy(), AN.copy()]
        _merge(s, cur, *raised(cur, 0.05), "cold", valid=False)
        assert s.dense_filter_state() == 1
        _merge(s, cur, *raised(cur, 0.05), "build")
        for k in range(3):
            _merge(s, cur, *raised(cur, 0.05), f"filtered {k}")
        _merge(s, cur, cur[0] - 1, cur[1] - 1, "below")
        _merge(s, cur, cur[0].copy(), cur[1].copy(), "equal")
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1, 3])
def test_short_batch_then_all_keys(ctx, R):
    """An identity batch shorter than the store makes it valid (the clamp pass covers the rows behind the batch);
    a batch over all keys then raises cells in those rows."""
    n_rows = (G + 37) // R
    n_keys = n_rows + (G + 5) // R
    rng = np.random.default_rng(77 + R)
    AP, AN = np.minimum(_cells(rng, n_keys, R), 2 ** 31 - 100), np.minimum(_cells(rng, n_keys, R), 2 ** 31 - 100)
    s = jg.PNCStore(ctx, n_keys, R, 8)
    try:
        s.write_rows(AP, AN)
        cur = [AP.copy(), AN.copy()]
        _merge(s, cur, AP[:n_rows] + 1, AN[:n_rows] - 1, "short, cold", valid=False)
        _merge(s, cur, AP[:n_rows] + 2, AN[:n_rows] + 2, "short, build")
        _merge(s, cur, AP[:n_rows] + 1, AN[:n_rows] + 3, "short, filtered")
        BP, BN = cur[0] - 1, cur[1] - 1
        BP[n_rows:, 0] += 5  # raised cells behind the first batch's rows, P and N
        BN[-1, :] += 7
        BN[n_rows, -1] += 2
        _merge(s, cur, BP, BN, "all keys")
        _merge(s, cur, BP, BN, "all keys, again")
        _merge(s, cur, cur[0] + 1, cur[1] + 1, "all keys, every cell")
    finally:
        s.close()


# ---- change patterns in the valid state ----------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("side", ["P", "N"])
def test_change_patterns_valid_state(ctx, side):
    """Nothing raised; one raised cell on each side of every line boundary (every wave and workgroup boundary is one);
    every cell raised.  After each a batch below the raised values changes nothing and one above wins: these merges
    read only the shadow, so they pass only if it was updated together with A."""
    n = 2 * G + 7
    assert n > 2 * G > 2 * WAVE > 2 * LINE
    rng = np.random.default_rng(5 if side == "P" else 6)
    AP, AN = np.minimum(_cells(rng, n, 1), 2 ** 31 - 1000), np.minimum(_cells(rng, n, 1), 2 ** 31 - 1000)
    w = 0 if side == "P" else 1
    s = jg.PNCStore(ctx, n, 1, 8)
    try:
        _make_valid(s, AP, AN)
        cur = [AP.copy(), AN.copy()]
        edge = np.zeros((n, 1), bool)
        for b in range(LINE, n, LINE):
            edge[b - 1, 0] = edge[b, 0] = True
        for name, mask in (("none", np.zeros((n, 1), bool)), ("edges", edge), ("all", np.ones((n, 1), bool))):
            B = [cur[0] - 1, cur[1] - 1]
            B[w][mask] += 11  # raised by 10
            _merge(s, cur, B[0], B[1], name)
            B = [cur[0] - 1, cur[1] - 1]
            B[w][mask] -= 4  # below the raised values, above the earlier ones
            _merge(s, cur, B[0], B[1], name + ", below")
            B = [cur[0] - 1, cur[1] - 1]
            B[w][mask] += 2
            B[w][::97] += 3
            _merge(s, cur, B[0], B[1], name + ", above")
    finally:
        s.close()


# ---- escapes ---------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("via", ["build", "filtered"])
def test_escape_cells(ctx, via):
    """A at and beyond both clamp values against B below, equal and above: every ordered pair of the edge values,
    laid out so that a 128-B line mixes escapes, known cells and raised cells; through the build launch (the pairs
    arrive at the second merge) and the filtered kernel (at the third), then a second batch of pairs by the shadow."""
    a = np.repeat(np.array(EDGES, np.int64), len(EDGES))
    b = np.tile(np.array(EDGES, np.int64), len(EDGES))
    pad = G + 9 - a.size % G  # past one workgroup, an odd total
    rng = np.random.default_rng(9)
    fill = rng.integers(0, 1000, pad).astype(np.int64)
    AP = np.concatenate([a, fill])[:, None]
    AN = np.concatenate([fill, a[::-1]])[:, None]
    BP = np.concatenate([b, fill + rng.integers(-1, 2, pad)])[:, None]
    BN = np.concatenate([fill + rng.integers(-1, 2, pad), b])[:, None]
    absent = np.full_like(AP, I64_MIN)
    s = jg.PNCStore(ctx, AP.shape[0], 1, 8)
    try:
        s.write_rows(AP, AN)
        cur = [AP.copy(), AN.copy()]
        _merge(s, cur, absent, absent, "cold", valid=False)
        if via == "filtered":
            _merge(s, cur, absent, absent, "build of the escapes")
        _merge(s, cur, BP, BN, via)
        _merge(s, cur, BP, BN, "again")
        _merge(s, cur, np.roll(BP, 5, 0), np.roll(BN, 7, 0), "rolled pairs")
        _merge(s, cur, absent, absent, "absent")
        _merge(s, cur, np.full_like(AP, I32_MAX), np.full_like(AP, I32_MIN), "clamp values")
        _merge(s, cur, np.full_like(AP, 2 ** 31), np.full_like(AP, I32_MAX - 1), "around INT32_MAX")
        _merge(s, cur, np.full_like(AP, I64_MAX), np.full_like(AP, I64_MAX), "INT64_MAX")
    finally:
        s.close()


# ---- every writer drops the shadow -----------------------------------------------------------------------------------

N_KEYS, R8 = 160, 8  # 1280 cells: past one workgroup


def _old():
    a = 1000 + np.arange(N_KEYS * R8, dtype=np.int64).reshape(N_KEYS, R8)
    return a, a + 5


def _w_write_rows(s, cur):
    cur[0] -= 600
    cur[1] -= 600
    s.write_rows(cur[0], cur[1])


def _w_write_rows_keyed(s, cur):
    k = np.array([3, 7, 79], np.uint32)
    cur[0][k] -= 600
    cur[1][k] -= 600
    s.write_rows(cur[0][k], cur[1][k], k)


def _ops():
    key = np.array([0, 5, 5, 40, 79], np.uint32)
    col = np.array([0, 2, 7, 3, 7], np.uint32)
    is_n = np.array([0, 1, 0, 1, 0], np.uint8)
    return key, col, is_n


def _w_apply_ops_negative(s, cur):
    key, col, is_n = _ops()
    s.apply_ops(key, col, np.full(key.size, -600, np.int64), is_n)
    for k, c, n in zip(key, col, is_n):
        cur[n][k, c] -= 600


def _w_apply_ops_wrap(s, cur):
    key, col, is_n = _ops()
    s.apply_ops(key, col, np.full(key.size, I64_MAX, np.int64), is_n)
    for k, c, n in zip(key, col, is_n):
        cur[n][k, c] = int(cur[n][k, c]) + I64_MAX - 2 ** 64  # the unchecked '+=' wraps below zero


def _w_apply_ops_rewind(s, cur):
    key = np.array([1, 1, 30, 79], np.uint32)
    is_n = np.array([0, 1, 0, 1], np.uint8)
    s.apply_ops_rewind(key, np.full(4, -600, np.int64), is_n, np.zeros(4, np.uint8), col=2)
    for k, n in zip(key, is_n):
        cur[n][k, 2] -= 600


LOWERING = {"write_rows": _w_write_rows, "write_rows_keyed": _w_write_rows_keyed, "apply_ops_negative": _w_apply_ops_negative,
            "apply_ops_wrap": _w_apply_ops_wrap, "apply_ops_rewind": _w_apply_ops_rewind}


def _between(s, old, cur):
    """Three dense merges of a batch that lies between the new and the old value wherever a cell changed (below the
    value elsewhere): the batch's values must win there.  A stale shadow would hold the old values."""
    B = []
    for o, c in zip(old, cur):
        b = c - 1
        ch = c != o
        lo, hi = np.minimum(c, o), np.maximum(c, o)
        b[ch] = lo[ch] // 2 + hi[ch] // 2  # strictly between: the values differ by hundreds
        B.append(b)
    for k in range(3):
        _merge(s, cur, B[0], B[1], f"between, merge {k}", valid=False)
    assert s.dense_filter_state() == 2


@pytest.mark.gpu
@pytest.mark.parametrize("writer", sorted(LOWERING))
def test_lowering_writers_drop_the_shadow(ctx, writer):
    old = _old()
    s = jg.PNCStore(ctx, N_KEYS, R8, 8)
    try:
        _make_valid(s, *old)
        cur = [old[0].copy(), old[1].copy()]
        LOWERING[writer](s, cur)
        assert s.dense_filter_state() == 0
        _same(s, cur[0], cur[1], writer)
        _between(s, old, cur)
    finally:
        s.close()


def _r_merge_rows_keyed(ctx, s, cur, k, BP, BN):
    s.merge_rows(BP, BN, k)


def _r_merge_batch_keyed(ctx, s, cur, k, BP, BN):
    b = jg.Rows(ctx, k.size, R8, 8)
    try:
        b.upload(BP, BN, k)
        s.merge_batch(b)
    finally:
        b.close()


def _r_merge_device(ctx, s, cur, k, BP, BN):
    import torch
    dev = torch.device("cuda", ctx.device)
    dk = torch.from_numpy(k.astype(np.int32)).to(dev)
    dP, dN = torch.from_numpy(BP).to(dev), torch.from_numpy(BN).to(dev)
    torch.cuda.synchronize(dev)
    s.merge_device(k.size, dk.data_ptr(), dP.data_ptr(), dN.data_ptr())


RAISING = {"merge_rows_keyed": _r_merge_rows_keyed, "merge_batch_keyed": _r_merge_batch_keyed, "merge_device": _r_merge_device}


@pytest.mark.gpu
@pytest.mark.parametrize("writer", sorted(RAISING))
def test_raising_writers_drop_the_shadow(ctx, writer):
    """Keyed merges raise cells by 1000: the state reads cold, and dense merges of a batch 500 above the old values
    leave the raised cells alone (a stale shadow would write the line back from the old values)."""
    old = _old()
    s = jg.PNCStore(ctx, N_KEYS, R8, 8)
    try:
        _make_valid(s, *old)
        cur = [old[0].copy(), old[1].copy()]
        k = np.array([2, 41, 2, 79], np.uint32)
        BP, BN = old[0][k] + 1000, old[1][k] - 1
        BN[:, 3] = old[1][k, 3] + 1000
        RAISING[writer](ctx, s, cur, k, BP, BN)
        np.maximum.at(cur[0], k, BP)
        np.maximum.at(cur[1], k, BN)
        assert s.dense_filter_state() == 0
        _same(s, cur[0], cur[1], writer)
        _between(s, old, cur)
    finally:
        s.close()


def _interned(ctx, rng):
    """A valid store whose keys' column 0 belongs to a known replica (the wire-format paths address cells by Guid)."""
    old = _old()
    s = jg.PNCStore(ctx, N_KEYS, R8, 8)
    guids = random_guids(rng, N_KEYS)
    cols = s.intern(np.arange(N_KEYS, dtype=np.uint32), [g[0] for g in guids], [g[1] for g in guids])
    assert (cols == 0).all()
    _make_valid(s, *old)
    return s, old, guids


@pytest.mark.gpu
def test_json_paths_drop_the_shadow(ctx):
    """jg_pnc_merge_json raising cells; a wave that fails after its fused apply (the undo takes the raises back); a
    streamed wave aborted after its appends: each leaves the store cold and the later dense merges exact."""
    rng = np.random.default_rng(21)
    s, old, guids = _interned(ctx, rng)
    try:
        cur = [old[0].copy(), old[1].copy()]
        keys = np.array([0, 9, 79], np.uint32)
        msgs = [encode_pnc([guids[k]], [int(old[0][k, 0]) + 1000], [int(old[1][k, 0]) + 1000]) for k in keys]
        s.merge_json(keys, msgs)
        for k in keys:
            cur[0][k, 0] += 1000
            cur[1][k, 0] += 1000
        assert s.dense_filter_state() == 0
        _same(s, cur[0], cur[1], "merge_json")
        _between(s, old, cur)

        base = [cur[0].copy(), cur[1].copy()]
        msgs = [encode_pnc([guids[k]], [int(cur[0][k, 0]) + 1000], [int(cur[1][k, 0]) + 1000]) for k in keys]
        with pytest.raises(jg.JanusError):
            s.merge_json(np.append(keys, 5).astype(np.uint32), msgs + [b'{"pVector":{},"nVector":{}'])
        assert s.dense_filter_state() == 0
        _same(s, cur[0], cur[1], "failed wave undone")
        B = [cur[0] - 1, cur[1] - 1]
        for k in keys:
            B[0][k, 0] += 501
            B[1][k, 0] += 501
        for k in range(3):
            _merge(s, cur, B[0], B[1], f"after the undo, merge {k}", valid=False)
        assert s.dense_filter_state() == 2 and not np.array_equal(cur[0], base[0])

        msgs = [encode_pnc([guids[k]], [int(cur[0][k, 0]) + 1000], [int(cur[1][k, 0]) + 1000]) for k in keys]
        s.wave_begin(16, 1 << 16)
        s.wave_append(keys, msgs)
        s.wave_abort()
        assert s.dense_filter_state() == 0
        _same(s, cur[0], cur[1], "aborted wave")
        for k in keys:
            B[0][k, 0] += 500
            B[1][k, 0] += 500
        for k in range(3):
            _merge(s, cur, B[0], B[1], f"after the abort, merge {k}", valid=False)
        assert s.dense_filter_state() == 2
    finally:
        s.close()


@pytest.mark.gpu
def test_node_wave_drops_the_shadow(ctx):
    """A committed node wave (jg_apply_committed) reaches the store without its public entry points."""
    rng = np.random.default_rng(22)
    old = _old()
    s = jg.PNCStore(ctx, N_KEYS, R8, 8)
    node = jg.Node(s, None)
    try:
        uids = random_guids(rng, N_KEYS)
        node.register([u[0] for u in uids], [u[1] for u in uids], [0] * N_KEYS, list(range(N_KEYS)))
        _make_valid(s, *old)
        cur = [old[0].copy(), old[1].copy()]
        keys = [4, 33, 79]
        msgs = [encode_pnc([(5, 7)], [int(old[0][k, 0]) + 1000], [int(old[1][k, 0]) + 1000]) for k in keys]
        done, cut, rc = node.apply_committed(None, [uids[k][0] for k in keys], [uids[k][1] for k in keys], [1] * len(keys), None, msgs)
        assert cut is None
        for k in keys:  # the wave's replica takes the key's first column
            cur[0][k, 0] += 1000
            cur[1][k, 0] += 1000
        assert s.dense_filter_state() == 0
        _same(s, cur[0], cur[1], "node wave")
        _between(s, old, cur)
    finally:
        node.close()
        s.close()


@pytest.mark.gpu
def test_synth_drops_the_shadow(ctx):
    """jg_synth_pnc_store rewrites every cell below the old values; a batch one above the new ones must win."""
    s = jg.PNCStore(ctx, N_KEYS, R8, 8)
    try:
        old = np.full((N_KEYS, R8), 2 ** 31 - 5, np.int64)
        _make_valid(s, old, old)
        s.synth(12345)
        assert s.dense_filter_state() == 0
        P, N = s.read_rows()
        assert P.max() < 2 ** 31 - 5 and (P != old).any()
        cur = [P.copy(), N.copy()]
        for k in range(3):
            _merge(s, cur, P + 1, N + 1, f"merge {k}", valid=False)
        assert np.array_equal(cur[0], P + 1) and s.dense_filter_state() == 2
    finally:
        s.close()


@pytest.mark.gpu
def test_reserve_drops_the_shadow(ctx):
    """jg_pnc_reserve in both dimensions: the shadow goes with the shape, the next dense merges start over at the
    new one and raise old and new cells alike."""
    old = _old()
    s = jg.PNCStore(ctx, N_KEYS, R8, 8)
    try:
        _make_valid(s, *old)
        cur = [old[0].copy(), old[1].copy()]
        for n_keys, R in ((N_KEYS + 50, R8), (N_KEYS + 50, 2 * R8)):
            s.reserve(n_keys, R)
            assert s.dense_filter_state() == 0
            grown = []
            for c in cur:
                g = np.zeros((n_keys, R), np.int64)
                g[:c.shape[0], :c.shape[1]] = c
                grown.append(g)
            cur = grown
            _same(s, cur[0], cur[1], ("reserve", n_keys, R))
            for k in range(3):
                BP, BN = cur[0] - 1, cur[1] - 1
                BP[::3] += 4
                BN[:, -1] += 9
                _merge(s, cur, BP, BN, ("reserve", n_keys, R, k), valid=False)
            assert s.dense_filter_state() == 2
    finally:
        s.close()
