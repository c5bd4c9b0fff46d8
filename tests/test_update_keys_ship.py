"""CPU-only: the surface of the client writes by key name that ship every snapshot (jg_node_update_keys_ship,
jg_node_shipped): both libraries export both symbols, the binding's signatures have one entry per parameter the header
declares, and the binding's export list is the header's function list."""
import ctypes
import inspect
import re
from pathlib import Path

import janus_gpu as jg

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "janus_gpu.h").read_text()
SHIP, SHIPPED = "jg_node_update_keys_ship", "jg_node_shipped"


def declaration(name):
    return [p.strip() for p in re.search(r"^int %s\((.*?)\);" % name, HEADER, flags=re.M | re.S).group(1).split(",")]


def test_both_libraries_export_both_symbols():
    for path in (jg.LIB_PATH, jg.LIB_PATH.with_name("libjanusgpu_test.so")):
        lib = ctypes.CDLL(str(path))
        for name in (SHIP, SHIPPED):
            assert hasattr(lib, name), (path, name)
    assert SHIP in jg.EXPORTS and SHIPPED in jg.EXPORTS


def test_signatures_have_one_entry_per_header_parameter():
    """jg_node_update_keys_encode's parameters without add_lim / rem_lim, n_bytes in front of out, n_rounds last: 26; and 4."""
    params, enc = declaration(SHIP), declaration("jg_node_update_keys_encode")
    assert len(params) == 26 and len(declaration(SHIPPED)) == 4
    assert params[:20] == enc[:20]  # node .. guid
    assert params[20:] == ["uint64_t* snap_off", "uint64_t* n_bytes", "uint8_t* out", "uint64_t cap", "uint8_t* sha", "uint32_t* n_rounds"]
    assert not any("add_lim" in p or "rem_lim" in p for p in params)
    args, res = jg._SIGS[SHIP]
    assert len(args) == 26 and res is ctypes.c_int
    assert args[2] is ctypes.c_uint64 and args[12] is ctypes.c_uint32 and args[23] is ctypes.c_uint64
    assert all(a is ctypes.c_void_p for i, a in enumerate(args) if i not in (2, 12, 23))
    assert declaration(SHIPPED) == ["jg_node* node", "uint64_t* n_bytes", "uint8_t* out", "uint64_t cap"]
    args, res = jg._SIGS[SHIPPED]
    assert len(args) == 4 and res is ctypes.c_int and args[3] is ctypes.c_uint64
    assert all(a is ctypes.c_void_p for a in args[:3])


def test_exports_equal_the_header():
    src = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert sorted(jg.EXPORTS) == sorted(set(re.findall(r"^\s*int\s+(jg_\w+)\s*\(", src, flags=re.M)))


def test_the_header_states_the_rules_and_the_limit_is_lifted():
    doc = HEADER[HEADER.index("Client writes by key name that ship every snapshot"):HEADER.index("int %s(" % SHIP)]
    for text in ("additive to ABI v10", "Rounds.", "n_rounds", "HOLDS", "jg_node_shipped", "ONCE ROUND 0 HAS WRITTEN", "JG_ESTATE", "snap[i] == 1",
                 "snap[i] == 2"):
        assert text in doc, text
    assert "LIMIT: OR-Set commands" not in HEADER and "get no bytes here" not in HEADER


def test_the_wrappers_take_what_the_issue_names():
    sig = inspect.signature(jg.Node.update_keys_ship)
    for name in ("keyspace", "keys", "ops", "args", "snap", "tags", "col", "sha", "cap"):
        assert name in sig.parameters, name
    assert sig.parameters["snap"].default is None and sig.parameters["cap"].default is None and sig.parameters["sha"].default is False
    assert callable(jg.Node.shipped)
