"""csrc/layout.hpp, the HIP-free half of the shared host plumbing: build/test_layout (host/test_layout.cpp, built by
`make all` with g++) checks the scratch layout builder, pow2_at_least and the checked narrowings on the CPU."""
import subprocess
from pathlib import Path


def test_layout_helpers_on_cpu():
    """The layout builder over counts 0, 1 and 2^31 + 5 at alignments 8, 16 and 256 (aligned offsets, no overlap, a
    total that covers the last array, zero-count arrays that take only padding and bind to a usable pointer);
    pow2_at_least at its floor, at a power of two and one past it; blocks_for at 0, 1, block, block + 1 and failing
    (not wrapping) past 2^31 - 1 workgroups; cub_count at INT_MAX and INT_MAX + 1."""
    exe = Path(__file__).resolve().parents[1] / "janus-crdt_amd" / "build" / "test_layout"
    assert exe.exists(), "built by __graft_entry__.build()"
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split("\n")
    for check in ("layout", "pow2_at_least", "blocks_for", "cub_count"):
        assert "ok " + check in lines, out.stdout
    assert lines[-2].startswith("PASS "), out.stdout
