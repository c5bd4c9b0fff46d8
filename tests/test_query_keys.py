"""CPU-only: the surface of the client reads by key name (jg_node_query_keys): the library exports it, the binding's
status constants are the header's, and the binding packs keys, elements and flags as the header lays them out."""
import ctypes
import re
from pathlib import Path

import numpy as np

import janus_gpu as jg

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "janus_gpu.h").read_text()


def test_library_exports_the_symbol():
    for path in (jg.LIB_PATH, jg.LIB_PATH.with_name("libjanusgpu_test.so")):
        assert hasattr(ctypes.CDLL(str(path)), "jg_node_query_keys"), path
    assert "jg_node_query_keys" in jg.EXPORTS and len(jg._SIGS["jg_node_query_keys"][0]) == 12


def test_status_constants_equal_the_header():
    defines = dict(re.findall(r"^#define\s+(JG_Q_\w+)\s+(\d+)", HEADER, flags=re.M))
    assert sorted(defines) == ["JG_Q_NO_ARG", "JG_Q_NO_CRDT", "JG_Q_NO_KEY", "JG_Q_OK", "JG_Q_OVERFLOW"]
    for name, v in defines.items():
        assert getattr(jg, name) == int(v), name
    assert (jg.Q_PNCOUNTER, jg.Q_ORSET, jg.Q_UNRESOLVED) == (0, 1, 255)


def test_packing_of_a_hand_made_batch():
    keys = ["a", b"", "schlüssel", b"k\0z"]
    elems = [None, "é", jg.NULL_ARG, b""]
    koff, kdata, eoff, edata, flag = jg.pack_queries(keys, elems)
    assert koff.dtype == np.uint64 and koff.tolist() == [0, 1, 1, 11, 14]
    assert kdata.dtype == np.uint8 and kdata.tobytes() == b"a" + "schlüssel".encode() + b"k\0z"
    assert eoff.dtype == np.uint64 and eoff.tolist() == [0, 0, 2, 2, 2]  # no argument and null carry no bytes
    assert edata.tobytes() == "é".encode()
    assert flag.dtype == np.uint8 and flag.tolist() == [0, 1, 2, 1]  # "" is a string (flag 1), not an absent argument
    # no query carries an argument: all three elem arrays are absent
    koff2, kdata2, eoff2, edata2, flag2 = jg.pack_queries(keys)
    assert koff2.tolist() == koff.tolist() and kdata2.tobytes() == kdata.tobytes() and eoff2 is edata2 is flag2 is None
    # elements without a byte still give three pointers
    _, _, eoff3, edata3, flag3 = jg.pack_queries(["x", "y"], [b"", jg.NULL_ARG])
    assert eoff3.tolist() == [0, 0, 0] and edata3.size >= 1 and flag3.tolist() == [1, 2]
    assert jg.pack_queries([], [])[0].tolist() == [0]
