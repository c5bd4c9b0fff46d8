"""Client writes by key name ON THE DEVICE against the oracle's SafeCRDT.Update (janus-crdt_amd/host/kat_update.cpp):
four nodes learn their keys through Receive and take a scripted batch of commands by key name on their prospective
copies through the host mirror's UpdateKeys (one jg_node_update_keys): increments, decrements, Add / Remove / Clear, the
null element, an unknown key, arguments of the wrong type and operation ids no wrapper knows.  Per command the status
and result are the oracle's; afterwards every key's "gp" equals QueryProspective and every encoded state equals
GetLastSynchronizedUpdate().Encode() byte for byte, also after further ops through the mirror's own ApplyOps; "gs" stays
as it was until a committed wave."""
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

BIN = Path(__file__).resolve().parent.parent / "janus-crdt_amd" / "build" / "kat_update"
SCENARIOS = ["Update.FourNodeWritesByName"]


def test_writes_by_name_equal_the_oracle_on_four_nodes():
    out = subprocess.run([str(BIN)], capture_output=True, text=True, timeout=110)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    passed = {line.split()[1] for line in out.stdout.splitlines() if line.startswith("PASS ")}
    missing = [s for s in SCENARIOS if s not in passed]
    assert not missing, missing
