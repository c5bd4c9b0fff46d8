"""Client reads by key name ON THE DEVICE against the oracle's SafeCRDT.QueryProspective / QueryStable
(janus-crdt_amd/host/kat_query.cpp): four nodes learn their keys through Receive, take client ops on their
prospective copies and one committed wave on their stable copies, and answer "gp" and "gs" for every key by name
through the host mirror's QueryKeys (one jg_node_query_keys per copy).  Before the wave "gs" lags "gp"; after it
they agree on every node (KVStoreTests.cs:225-286)."""
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

BIN = Path(__file__).resolve().parent.parent / "janus-crdt_amd" / "build" / "kat_query"
SCENARIOS = ["Query.FourNodeReadsByName"]


def test_reads_by_name_equal_the_oracle_on_four_nodes():
    out = subprocess.run([str(BIN)], capture_output=True, text=True, timeout=110)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    passed = {line.split()[1] for line in out.stdout.splitlines() if line.startswith("PASS ")}
    missing = [s for s in SCENARIOS if s not in passed]
    assert not missing, missing
