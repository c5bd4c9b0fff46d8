"""Client writes by key name that ship every snapshot, OR-Set keys included, ON THE DEVICE against the oracle's
SafeCRDT.Update and its client batcher (janus-crdt_amd/host/kat_update_ship.cpp): four nodes take two scripted batches of
"a" / "r" / "c" / "i" commands by key name through the host mirror's UpdateKeysShip (one jg_node_update_keys_ship each),
with sets cleared after a shipped command, cleared twice in a row and cleared with nothing shipped before.  Safe updates:
every applied command's bytes and SHA-256, of either kind, are the message the oracle's SafeCRDT.Update handed its batcher
for that command.  Non-safe updates: the commands that ship are the objects ActualPropagateSyncMsg kept for the batch,
each with the bytes it kept.  "gp" / "gs" of every key are the oracle's, before and after a committed wave."""
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

BIN = Path(__file__).resolve().parent.parent / "janus-crdt_amd" / "build" / "kat_update_ship"
SCENARIOS = ["UpdateShip.FourNodeWritesThatShipEveryKind"]


def test_shipped_snapshots_equal_the_oracle_on_four_nodes():
    out = subprocess.run([str(BIN)], capture_output=True, text=True, timeout=110)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    passed = {line.split()[1] for line in out.stdout.splitlines() if line.startswith("PASS ")}
    missing = [s for s in SCENARIOS if s not in passed]
    assert not missing, missing
