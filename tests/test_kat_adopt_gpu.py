"""GPU: host/kat_adopt — four nodes whose rows and set ids the node allocates: creations by jg_node_create_uids, learnt
keys adopted by jg_node_adopt_keys (a late Create message included), one committed wave, and every key's "gp" / "gs" by
name against the oracle's SafeCRDTManager."""
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu


def test_kat_adopt_binary():
    exe = Path(__file__).resolve().parents[1] / "janus-crdt_amd" / "build" / "kat_adopt"
    assert exe.exists(), "built by __graft_entry__.build()"
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith(("PASS", "FAIL"))]
    assert out.returncode == 0 and len(lines) == 1 and all(ln.startswith("PASS") for ln in lines), out.stdout[-2000:] + out.stderr[-2000:]
