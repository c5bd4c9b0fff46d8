"""The edges of k_merge_dense's shape (csrc/pnc_dense_kernels.hpp): kDenseVecs 16-B vectors of each array per lane, kDenseBlock
lanes per workgroup, so a workgroup takes W = kDenseVecs x kDenseBlock vectors per trip, a wave-instruction reads
64 consecutive vectors, a lane's vectors lie kDenseBlock apart, an aligned group of 8 lanes is one 128-B line (written
whole or not at all), and the cells behind the last whole vector are block 0's.  P and N are merged by different
workgroups (the two halves of the grid), hence every edge with a raised cell in P only, in N only and in both.
Bit-exact against the oracle on the full P and N read back, as in test_pnc_elide_gpu.py.

Totals (in vectors): W - 1, W, W + 1, 2W + 7, a last trip of less than one wave (W + 37) and of less than one line
group (W + 3), each with and without trailing cells.  One column (R = 1) reaches every total exactly; R = 64 and
R = 7 cannot (a row is 64 or 7 cells), so they take the fewest rows that hold at least that many cells: the nearest
total from above, with whatever trailing cells that row count leaves (none at R = 64).

W and the block size are mirrored here as literals; test_constants_match_the_kernel (no GPU) reads the kernel's
constexpr lines, so a re-tune that forgets this file fails."""
import functools
import re
from pathlib import Path

import numpy as np
import pytest

import oracle_ref as orc
from gen import random_pnc

DENSE_VECS = 1     # kDenseVecs
DENSE_BLOCK = 256  # kDenseBlock
W = DENSE_VECS * DENSE_BLOCK

KERNELS_HPP = Path(__file__).resolve().parent.parent / "janus-crdt_amd" / "csrc" / "pnc_dense_kernels.hpp"


def test_constants_match_the_kernel():
    src = KERNELS_HPP.read_text()
    got = {}
    for name in ("kDenseVecs", "kDenseBlock"):
        m = re.findall(r"^constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, src, re.M)
        assert len(m) == 1, f"{name}: expected one `constexpr <type> {name} = <literal>;` line in csrc/pnc_dense_kernels.hpp"
        got[name] = int(m[0])
    assert got == {"kDenseVecs": DENSE_VECS, "kDenseBlock": DENSE_BLOCK}
    assert W == got["kDenseVecs"] * got["kDenseBlock"]


def _dt(eb):
    return np.int32 if eb == 4 else np.int64


TOTALS = [W - 1, W, W + 1, 2 * W + 7, W + 37, W + 3]  # in vectors


def _shapes():
    """(n_keys, R) per width: every total x {no trailing cell, one} exactly at R = 1, from above at R = 64 and 7."""
    out = {4: [], 8: []}
    for eb in (4, 8):
        per_vec = 16 // eb
        seen = set()
        for t in TOTALS:
            for trailing in (0, 1):
                cells = t * per_vec + trailing
                for R in (1, 64, 7):
                    shape = (-(-cells // R), R)
                    if shape not in seen:
                        seen.add(shape)
                        out[eb].append(shape)
    return out


SHAPES = _shapes()
CASES = [(n, R, eb) for eb in (4, 8) for n, R in SHAPES[eb]]


@functools.lru_cache(maxsize=None)
def _a(n_keys, R, eb):
    """The local state of a shape (shared by its cases, read-only): the width's whole range short of its maximum."""
    rng = np.random.default_rng(n_keys * 1009 + R * 31 + eb)
    info = np.iinfo(_dt(eb))
    AP = random_pnc(rng, n_keys, R, eb, absent=False, hi=info.max - 1)
    AN = random_pnc(rng, n_keys, R, eb, absent=False, hi=info.max - 1)
    AP.setflags(write=False)
    AN.setflags(write=False)
    return AP, AN


def _edge_cells(total, eb):
    """Flat cell indices on both sides of every boundary the shape creates: the first and last cell of each trip, of
    a wave-instruction (64 vectors) and of a 128-B line (8 vectors) at the start of a trip and around the last whole
    vector's; the step from a lane's first vector to its second (kDenseBlock vectors on, where kDenseVecs > 1); the
    last whole vector and the first trailing cell."""
    per_vec = 16 // eb
    nv = total // per_vec
    vecs = set()
    for trip0 in range(0, nv + 1, W):
        for v in (0, 7, 8, 63, 64, DENSE_BLOCK - 1, DENSE_BLOCK, W - 1):
            vecs.add(trip0 + v)
    last = nv - 1
    for v in (last, last - last % 8, last - last % 8 - 1, last - last % 64, last - last % 64 - 1):
        vecs.add(v)
    cells = {0, total - 1, nv * per_vec}  # nv * per_vec: the first trailing cell
    for v in vecs:
        if 0 <= v < nv:
            cells.update((v * per_vec, v * per_vec + per_vec - 1))
    return sorted(c for c in cells if 0 <= c < total)


def _below(rng, A, p_absent=0.3):
    info = np.iinfo(A.dtype)
    B = np.minimum(A, random_pnc(rng, A.shape[0], A.shape[1], A.dtype.itemsize, absent=False))
    B[rng.random(A.shape) < p_absent] = info.min
    return B


def _raise(rng, A, p):
    B = _below(rng, A)
    m = rng.random(A.shape) < p
    B[m] = A[m] + 1
    return B


def _batches(n_keys, R, eb):
    """(name, BP, BN): equal to A, all ABSENT, 1 % and 50 % of the cells raised, one raised cell per edge in P and N,
    N only and P only."""
    AP, AN = _a(n_keys, R, eb)
    rng = np.random.default_rng(n_keys * 7 + R + eb)
    info = np.iinfo(_dt(eb))
    yield "equal", AP.copy(), AN.copy()
    yield "absent", np.full_like(AP, info.min), np.full_like(AN, info.min)
    for p in (0.01, 0.5):
        yield f"random {p}", _raise(rng, AP, p), _raise(rng, AN, p)
    for c in _edge_cells(n_keys * R, eb):
        for in_p, in_n in ((True, True), (False, True), (True, False)):
            BP, BN = AP.copy(), AN.copy()
            if in_p:
                BP.flat[c] += 1
            if in_n:
                BN.flat[c] += 1
            yield f"cell {c} P={in_p} N={in_n}", BP, BN


def _ids(case):
    return "%dx%d-eb%d" % case


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_merge_rows(ctx, case):
    """Every batch on a fresh A through jg_pnc_merge_rows, then once more: the state stays."""
    import janus_gpu as jg
    n_keys, R, eb = case
    AP, AN = _a(n_keys, R, eb)
    s = jg.PNCStore(ctx, n_keys, R, eb)
    try:
        for name, BP, BN in _batches(n_keys, R, eb):
            eP, eN = orc.pnc_merge(AP, AN, BP, BN)
            s.write_rows(AP, AN)
            for again in (False, True):
                s.merge_rows(BP, BN)
                P, N = s.read_rows()
                assert np.array_equal(P, eP) and np.array_equal(N, eN), (name, again)
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_merge_batch_device_rows(ctx, case):
    """The same through Rows.upload + merge_batch(async_=True), the benchmark's call."""
    import janus_gpu as jg
    n_keys, R, eb = case
    AP, AN = _a(n_keys, R, eb)
    s = jg.PNCStore(ctx, n_keys, R, eb)
    b = jg.Rows(ctx, n_keys, R, eb)
    try:
        for name, BP, BN in _batches(n_keys, R, eb):
            eP, eN = orc.pnc_merge(AP, AN, BP, BN)
            s.write_rows(AP, AN)
            b.upload(BP, BN)
            for again in (False, True):
                s.merge_batch(b, async_=True)
                ctx.fence()
                P, N = s.read_rows()
                assert np.array_equal(P, eP) and np.array_equal(N, eN), (name, again)
    finally:
        s.close()
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("eb", [4, 8])
@pytest.mark.parametrize("R", [64, 7])
def test_short_batch(ctx, R, eb):
    """A batch of fewer rows than the store has keys (its last trip partial, every cell raised): the rows behind it
    stay bit-identical, through both calls."""
    import janus_gpu as jg
    per_vec = 16 // eb
    n_rows = -(-((W + 37) * per_vec + 1) // R)
    n_keys = n_rows + -(-(W * per_vec) // R) + 3
    AP, AN = _a(n_keys, R, eb)
    BP, BN = AP[:n_rows] + 1, AN[:n_rows] + 1
    eP, eN = AP.copy(), AN.copy()
    eP[:n_rows], eN[:n_rows] = orc.pnc_merge(AP[:n_rows], AN[:n_rows], BP, BN)
    s = jg.PNCStore(ctx, n_keys, R, eb)
    b = jg.Rows(ctx, n_rows, R, eb)
    try:
        s.write_rows(AP, AN)
        s.merge_rows(BP, BN)
        P, N = s.read_rows()
        assert np.array_equal(P, eP) and np.array_equal(N, eN)
        s.write_rows(AP, AN)
        b.upload(BP, BN)
        s.merge_batch(b, async_=True)
        ctx.fence()
        P, N = s.read_rows()
        assert np.array_equal(P, eP) and np.array_equal(N, eN)
    finally:
        s.close()
        b.close()
