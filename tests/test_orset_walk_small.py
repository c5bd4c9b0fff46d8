"""CPU-only: the one-launch form of the OR-Set record walk (csrc/orset_walk_small.hip): its two entry
points in the library, the header and the binding, and the index arithmetic it adds (csrc/orset_walk_small.hpp) against
sequential restatements, plain and under the sanitizers."""
import ctypes
import re
import subprocess
from pathlib import Path

import pytest

import janus_gpu as jg

ROOT = Path(__file__).resolve().parent.parent
BUILD = ROOT / "janus-crdt_amd" / "build"
NAMES = ("jg_orset_set_walk_small", "jg_orset_walk_small_stats")


def test_library_exports_the_switch_and_the_witness():
    lib = ctypes.CDLL(str(jg.LIB_PATH))
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.jg_abi_version() == 10


def test_binding_matches_the_header():
    src = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "janus_gpu.h").read_text(), flags=re.S)
    for name in NAMES:
        m = re.search(r"^\s*int\s+%s\s*\(([^)]*)\)" % name, src, flags=re.M)
        assert m, name
        assert name in jg.EXPORTS
        assert len(jg._SIGS[name][0]) == len(m.group(1).split(","))
    assert "uint64_t out[6]" in src
    assert hasattr(jg.ORSetStore, "set_walk_small") and hasattr(jg.ORSetStore, "walk_small_stats")
    assert (jg.ORSetStore.WALK_SMALL_OFF, jg.ORSetStore.WALK_SMALL_ON, jg.ORSetStore.WALK_SMALL_AUTO) == (0, 1, 2)


def test_header_docs_cite_the_reference():
    text = (ROOT / "include" / "janus_gpu.h").read_text()
    for name in NAMES:
        doc = text[:text.index("int %s(" % name)].rsplit("/*", 1)[1]
        assert "ORSet.cs:134-198" in doc, name


def test_the_caps_hold_the_reference_batch():
    """clientBatchSize = 1000 commands must fit the one-launch form; the thresholds are plain numbers the GPU test reads."""
    hpp = (ROOT / "janus-crdt_amd" / "csrc" / "orset_walk_small.hpp").read_text()
    cap = int(re.search(r"kMaxOps = (\d+);", hpp).group(1))
    assert cap in (1024, 2048, 4096)
    internal = (ROOT / "janus-crdt_amd" / "csrc" / "jg_internal.hpp").read_text()
    assert re.search(r"kWalkSmallAutoMinOps = (\d+);", internal) and re.search(r"kWalkAutoMinOps = (\d+);", internal)
    assert int(re.search(r"kWalkAutoMinOps = (\d+);", internal).group(1)) <= 4096  # never raised


@pytest.mark.parametrize("exe", ["test_orset_walk_small", "test_orset_walk_small_san"])
def test_kernel_index_arithmetic(exe):
    out = subprocess.run([str(BUILD / exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok" in out.stdout
