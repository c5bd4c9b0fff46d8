"""A client stream with its "gp" reads in order among the writes ON THE DEVICE against the oracle's SafeCRDT.Update and
SafeCRDT.QueryProspective run one by one (janus-crdt_amd/host/kat_exec.cpp): kat_update_ship's four nodes take its two
scripted batches by key name through the host mirror's ExecKeys (one jg_node_exec_keys each) with a read of the same key
behind every command.  Every read's status and value are QueryProspective's at that point of the stream; every applied
write's bytes and SHA-256 are the message SafeCRDT.Update handed its batcher (safe), or the objects the batcher kept
(non-safe).  "gp" / "gs" of every key are the oracle's, before and after a committed wave."""
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

BIN = Path(__file__).resolve().parent.parent / "janus-crdt_amd" / "build" / "kat_exec"
SCENARIOS = ["Exec.FourNodeStreamsWithReadsInOrder"]


def test_streams_with_reads_equal_the_oracle_on_four_nodes():
    out = subprocess.run([str(BIN)], capture_output=True, text=True, timeout=110)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    passed = {line.split()[1] for line in out.stdout.splitlines() if line.startswith("PASS ")}
    missing = [s for s in SCENARIOS if s not in passed]
    assert not missing, missing
