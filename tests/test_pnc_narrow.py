"""csrc/pnc_filter.hpp's narrow form of a received int64 cell (fits, narrow, widen), on the CPU: build/test_pnc_narrow
(host/test_pnc_narrow.cpp, built by `make all` with g++) checks the three functions, their round trips and the merge
of every store cell among the edge values INT64_MIN, INT32_MIN - 1, INT32_MIN, INT32_MIN + 1, -1, 0, 1, INT32_MAX - 1,
INT32_MAX, 2^31, 2^40, INT64_MAX with every fitting received cell that arrives as its 4-byte code, against plain int64
max; build/test_pnc_narrow_san is the same program under the address and undefined-behaviour sanitizers, a
stand-alone process."""
import subprocess
from pathlib import Path

import pytest

BUILD = Path(__file__).resolve().parents[1] / "janus-crdt_amd" / "build"


@pytest.mark.parametrize("exe", ["test_pnc_narrow", "test_pnc_narrow_san"])
def test_narrow_form_on_cpu(exe):
    """A cell fits if it is ABSENT or in (INT32_MIN, INT32_MAX]; the reserved code INT32_MIN is ABSENT's, so a real
    INT32_MIN does not fit; widen(narrow(b)) == b; a merge by the widened code is the merge by the cell."""
    path = BUILD / exe
    assert path.exists(), "built by __graft_entry__.build()"
    out = subprocess.run([str(path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split("\n")
    for check in ("fits", "roundtrip", "pairs"):
        assert "ok " + check in lines, out.stdout
    assert lines[-2].startswith("PASS "), out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
