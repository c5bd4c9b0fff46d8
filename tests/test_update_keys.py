"""CPU-only: the surface of the client writes by key name (jg_node_update_keys): both libraries export it, the binding's
signature has one entry per parameter the header declares, its status constants are the header's, and pack_commands lays
keys, ops, flags, amounts and elements out as the header reads them."""
import ctypes
import re
from pathlib import Path

import numpy as np

import janus_gpu as jg

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "janus_gpu.h").read_text()


def test_library_exports_the_symbol():
    for path in (jg.LIB_PATH, jg.LIB_PATH.with_name("libjanusgpu_test.so")):
        assert hasattr(ctypes.CDLL(str(path)), "jg_node_update_keys"), path
    assert "jg_node_update_keys" in jg.EXPORTS


def test_signature_has_one_entry_per_header_parameter():
    """The header declares 21 parameters (node, ks, n, 2 key arrays, op, arg_flag, amount, 2 element arrays, 2 tag arrays,
    col, 8 outputs); the binding's table has one ctypes entry for each, col the only 32-bit scalar."""
    decl = re.search(r"^int jg_node_update_keys\((.*?)\);", HEADER, flags=re.M | re.S).group(1)
    params = [p.strip() for p in decl.split(",")]
    assert len(params) == 21 and params[12] == "uint32_t col" and params[2] == "uint64_t n"
    args, res = jg._SIGS["jg_node_update_keys"]
    assert len(args) == len(params) and res is ctypes.c_int
    assert args[2] is ctypes.c_uint64 and args[12] is ctypes.c_uint32
    assert all(a is ctypes.c_void_p for i, a in enumerate(args) if i not in (2, 12))


def test_status_constants_equal_the_header():
    defines = dict(re.findall(r"^#define\s+(JG_U_\w+)\s+(\d+)", HEADER, flags=re.M))
    assert sorted(defines) == ["JG_U_BAD_ARG", "JG_U_BAD_OP", "JG_U_NO_CRDT", "JG_U_NO_KEY", "JG_U_OK"]
    for name, v in defines.items():
        assert getattr(jg, name) == int(v), name
    assert jg.JG_U_OK == 0
    assert (jg.JG_U_NO_KEY, jg.JG_U_NO_CRDT) == (jg.JG_Q_NO_KEY, jg.JG_Q_NO_CRDT)  # they mean what the reads' mean


def test_packing_of_a_hand_made_batch():
    keys = ["a", b"", "schlüssel", b"k\0z", "n"]
    ops = [1, 2, 3, 1, 0]
    args = [7, "é", jg.NULL_ARG, b"", None]
    koff, kdata, op, flag, amount, eoff, edata = jg.pack_commands(keys, ops, args)
    assert koff.dtype == np.uint64 and koff.tolist() == [0, 1, 1, 11, 14, 15]
    assert kdata.dtype == np.uint8 and kdata.tobytes() == b"a" + "schlüssel".encode() + b"k\0zn"
    assert op.dtype == np.uint8 and op.tolist() == ops
    assert flag.dtype == np.uint8 and flag.tolist() == [3, 1, 2, 1, 0]  # "" is a string (flag 1), not an absent argument
    assert amount.dtype == np.int64 and amount.tolist() == [7, 0, 0, 0, 0]
    assert eoff.dtype == np.uint64 and eoff.tolist() == [0, 0, 2, 2, 2, 2]  # an integer, null and no argument carry no bytes
    assert edata.tobytes() == "é".encode()
    # a batch without strings: NULL element arrays; negative and 64-bit amounts survive
    _, _, _, flag2, amount2, eoff2, edata2 = jg.pack_commands(["x", "y", "z"], [1, 2, 3], [-5, np.int64(1 << 62), jg.NULL_ARG])
    assert flag2.tolist() == [3, 3, 2] and amount2.tolist() == [-5, 1 << 62, 0] and eoff2 is None and edata2 is None
    # a batch without integers: no amount array; strings without a byte still give both element pointers
    _, _, _, flag3, amount3, eoff3, edata3 = jg.pack_commands(["x", "y"], [1, 1], [b"", None])
    assert flag3.tolist() == [1, 0] and amount3 is None and eoff3.tolist() == [0, 0, 0] and edata3.size >= 1
    assert jg.pack_commands([], [], [])[0].tolist() == [0]
