"""CPU-only: the elastic PN-Counter store's ABI surface (jg_pnc_shape, jg_pnc_reserve, jg_pnc_set_max_replicas):
declared by the header, carried by the binding, exported by the library, and refusing a NULL handle with
JG_EINVAL before any device is touched.  The behaviour on a device is tests/test_pnc_reserve_gpu.py's."""
import ctypes as C
import re
from pathlib import Path

import janus_gpu as jg

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("jg_pnc_shape", "jg_pnc_reserve", "jg_pnc_set_max_replicas")


def test_header_binding_and_library_carry_the_names():
    src = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "janus_gpu.h").read_text(), flags=re.S)
    declared = set(re.findall(r"^\s*int\s+(jg_\w+)\s*\(", src, flags=re.M))
    lib = C.CDLL(str(jg.LIB_PATH))
    for name in NAMES:
        assert name in declared, name
        assert name in jg.EXPORTS, name
        assert hasattr(lib, name), name
    assert lib.jg_abi_version() == 10  # additive: the version stays


def test_header_cites_what_the_calls_stand_in_for():
    text = (ROOT / "include" / "janus_gpu.h").read_text()
    at = text.index("int jg_pnc_shape(")
    block = text[at:text.index("int jg_pnc_set_max_replicas(")]
    assert "PNCounters.cs:131-144" in block and "KeySpaceManager.cs:121-136" in block
    assert "resident together" in block  # the old and the new buffers during the call


def test_null_handle_is_einval_without_a_device():
    lib = jg.load()
    nk, r, eb = C.c_uint64(7), C.c_uint32(7), C.c_uint32(7)
    assert lib.jg_pnc_shape(None, C.byref(nk), C.byref(r), C.byref(eb)) == jg.JG_EINVAL
    assert (nk.value, r.value, eb.value) == (7, 7, 7)  # nothing written
    assert lib.jg_pnc_reserve(None, 10, 10) == jg.JG_EINVAL
    assert lib.jg_pnc_set_max_replicas(None, 8) == jg.JG_EINVAL
    buf = C.create_string_buffer(256)
    lib.jg_last_error(buf, 256)
    assert b"jg_pnc_set_max_replicas" in buf.value
