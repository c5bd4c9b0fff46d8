"""CPU-only: the surface of the client writes by key name that ship their PN-Counter snapshots
(jg_node_update_keys_encode): both libraries export it, the binding's signature has one entry per parameter the header
declares, the header documents the three snap values, and the binding's export list is the header's function list."""
import ctypes
import inspect
import re
from pathlib import Path

import janus_gpu as jg

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "janus_gpu.h").read_text()
NAME = "jg_node_update_keys_encode"


def declaration(name):
    return re.search(r"^int %s\((.*?)\);" % name, HEADER, flags=re.M | re.S).group(1)


def test_both_libraries_export_the_symbol():
    for path in (jg.LIB_PATH, jg.LIB_PATH.with_name("libjanusgpu_test.so")):
        assert hasattr(ctypes.CDLL(str(path)), NAME), path
    assert NAME in jg.EXPORTS


def test_signature_has_one_entry_per_header_parameter():
    """jg_node_update_keys' 21 parameters in its order, with snap behind col (the last input) and snap_off, out, cap and sha
    behind rem_lim (the last output): 26, col and cap the only scalars besides n."""
    params = [p.strip() for p in declaration(NAME).split(",")]
    base = [p.strip() for p in declaration("jg_node_update_keys").split(",")]
    assert len(params) == 26
    assert params[:13] == base[:13] and params[13] == "const uint8_t* snap" and params[14:22] == base[13:]
    assert params[22:] == ["uint64_t* snap_off", "uint8_t* out", "uint64_t cap", "uint8_t* sha"]
    args, res = jg._SIGS[NAME]
    assert len(args) == len(params) and res is ctypes.c_int
    assert args[2] is ctypes.c_uint64 and args[12] is ctypes.c_uint32 and args[24] is ctypes.c_uint64
    assert all(a is ctypes.c_void_p for i, a in enumerate(args) if i not in (2, 12, 24))


def test_header_documents_the_snap_values():
    doc = HEADER[HEADER.index("Client writes by key name that also ship"):HEADER.index("int %s(" % NAME)]
    for v in ("snap[i] == 0", "snap[i] == 1", "snap[i] == 2"):
        assert v in doc, v
    assert "ONE batcher batch" in doc and "LIMIT" in doc and "JG_ESTATE" in doc
    assert "additive to ABI v10" in doc


def test_exports_equal_the_header():
    src = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert sorted(jg.EXPORTS) == sorted(set(re.findall(r"^\s*int\s+(jg_\w+)\s*\(", src, flags=re.M)))


def test_the_wrapper_takes_what_the_issue_names():
    sig = inspect.signature(jg.Node.update_keys_encode)
    for name in ("keyspace", "keys", "ops", "args", "snap", "tags", "col", "sha", "cap"):
        assert name in sig.parameters, name
    assert sig.parameters["snap"].default is None and sig.parameters["cap"].default is None and sig.parameters["sha"].default is False
