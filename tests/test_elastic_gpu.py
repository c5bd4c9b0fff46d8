"""GPU: host/kat_elastic — four GpuStableStore nodes created for 2 keys x 2 replica columns with SetElastic(64, 16)
learn 8 keys through GpuKeySpace::Receive, create the counters from the callback (key growth 2 -> 8) and apply one
committed wave whose keys need 5 columns (2 -> 4 -> 8); values, column order and encoded states equal the oracle's,
jg_pnc_shape reports 8 x 8, and a store that never asked keeps its "PNCounter store full"."""
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu


def test_kat_elastic_binary():
    exe = Path(__file__).resolve().parents[1] / "janus-crdt_amd" / "build" / "kat_elastic"
    assert exe.exists(), "built by __graft_entry__.build()"
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith(("PASS", "FAIL"))]
    assert out.returncode == 0 and len(lines) == 2 and all(ln.startswith("PASS") for ln in lines), out.stdout[-2000:] + out.stderr[-2000:]
