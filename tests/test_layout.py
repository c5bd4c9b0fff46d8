"""csrc/layout.hpp, the HIP-free half of the shared host plumbing: build/test_layout (host/test_layout.cpp, built by
`make all` with g++) checks the scratch layout builder, pow2_at_least and the checked narrowings on the CPU, and
csrc/orset_layouts.hpp's three carved blocks of the OR-Set wave path against their formulas written out;
build/test_layout_san is the same program under the address and undefined-behaviour sanitizers, a stand-alone
process."""
import subprocess
from pathlib import Path

CHECKS = ("layout", "pow2_at_least", "blocks_for", "cub_count", "halves_of", "orset_layouts", "pnc_wave_layout")


def _run(name):
    exe = Path(__file__).resolve().parents[1] / "janus-crdt_amd" / "build" / name
    assert exe.exists(), "built by __graft_entry__.build()"
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split("\n")
    for check in CHECKS:
        assert "ok " + check in lines, out.stdout
    assert lines[-2].startswith("PASS "), out.stdout
    return out


def test_layout_helpers_on_cpu():
    """The layout builder over counts 0, 1 and 2^31 + 5 at alignments 8, 16 and 256 (aligned offsets, no overlap, a
    total that covers the last array, zero-count arrays that take only padding and bind to a usable pointer);
    pow2_at_least at its floor, at a power of two and one past it; blocks_for at 0, 1, block, block + 1 and failing
    (not wrapping) past 2^31 - 1 workgroups; cub_count at INT_MAX and INT_MAX + 1; halves_of (the dense PN-Counter merges'
    two-halves grid) for each (cells per unit, units per workgroup) pair the library launches at 0 cells, 1, a unit less
    one, one unit, a workgroup's cells - 1 / exactly / + 1, a count with trailing cells and the largest count that fits
    one launch (and one past it), and k_merge_dense's units against its byte arithmetic.  The OR-Set wave path's blocks:
    the claims' counts at caps 0, 1, 62, 63, 1023, 1024, 2^20 and 0x7FFFFFF0 - 1, the bucket commit's seven arrays at
    table sizes {4096, 2^20, 2^30}^2, the names staging at n in {0, 1, 3, 4, 5} x nb in {0, 1, 17} and its copy-out.
    The PN-Counter wave's status block (csrc/pnc_wave_layout.hpp) at n in {0, 1, 2, 3, 7, 8, 1000, 131072} and grown
    from each to the next: offsets and sizes, the roll-back slots inside the block, the capacity read back >= n, a
    grown block's deferred list where the old one was."""
    _run("test_layout")


def test_layout_helpers_under_sanitizers():
    """The same program built with -fsanitize=address,undefined: no report."""
    out = _run("test_layout_san")
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
