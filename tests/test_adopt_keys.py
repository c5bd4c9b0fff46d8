"""CPU-only: the surface of CRDT creation on the device (jg_node_next_idx, jg_node_create_uids, jg_node_adopt_keys) —
both libraries export the names, the binding's signatures have one entry per header parameter, its constants equal the
header's — and tests/adopt_ref.py, the model the GPU tests compare against, on cases worked out by hand."""
import ctypes
import re
from pathlib import Path

import pytest

import adopt_ref as A
import janus_gpu as jg

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "janus_gpu.h").read_text()
NAMES = ("jg_node_next_idx", "jg_node_create_uids", "jg_node_adopt_keys")


@pytest.mark.parametrize("lib", ["libjanusgpu.so", "libjanusgpu_test.so"])
def test_both_libraries_export_the_names(lib):
    h = ctypes.CDLL(str(jg.LIB_PATH.parent / lib))
    for name in NAMES:
        assert hasattr(h, name), (lib, name)
    assert h.jg_abi_version() == 10  # additive: the version stays


@pytest.mark.parametrize("name", NAMES)
def test_signature_has_one_entry_per_header_parameter(name):
    src = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    m = re.search(r"^\s*int\s+%s\s*\(([^)]*)\)\s*;" % name, src, flags=re.M)
    assert m, name
    params = [p.strip() for p in m.group(1).split(",")]
    args, ret = jg._SIGS[name]
    assert ret is ctypes.c_int and len(args) == len(params)
    for p, a in zip(params, args):
        if "*" in p:
            assert a is jg._vp or issubclass(a, ctypes._Pointer), (name, p)
        else:
            assert a is {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}[p.split()[0]], (name, p)
    assert name in jg.EXPORTS


def test_constants_equal_the_header():
    for name in ("JG_C_CREATED", "JG_C_EXISTS", "JG_A_ADOPTED", "JG_A_HAVE", "JG_A_NO_TYPE", "JG_A_SKIPPED"):
        m = re.search(r"^#define\s+%s\s+(\d+)" % name, HEADER, flags=re.M)
        assert m and int(m.group(1)) == getattr(jg, name), name
    assert (A.CREATED, A.EXISTS) == (jg.JG_C_CREATED, jg.JG_C_EXISTS)
    assert (A.ADOPTED, A.HAVE, A.NO_TYPE, A.SKIPPED) == (jg.JG_A_ADOPTED, jg.JG_A_HAVE, jg.JG_A_NO_TYPE, jg.JG_A_SKIPPED)
    assert (A.OK, A.EINVAL, A.ESTATE) == (jg.JG_OK, jg.JG_EINVAL, jg.JG_ESTATE)


U = [(k, 100 + k) for k in range(1, 20)]
REP = (7, 7)


def test_model_allocates_in_call_order_per_kind():
    m = A.NodeModel(n_keys=8, R=2)
    assert m.next == [0, 0]
    st, idx = m.create_uids(U[:5], [0, 1, 1, 0, 1])
    assert st == [A.CREATED] * 5 and idx == [0, 0, 1, 1, 2] and m.next == [2, 3]
    # a repeat inside the batch and a uid of an earlier call: the first creation stands, whatever type the repeat names
    st, idx = m.create_uids([U[5], U[0], U[5], U[6]], [1, 1, 0, 0])
    assert st == [A.CREATED, A.EXISTS, A.EXISTS, A.CREATED] and idx == [3, 0, 3, 2]
    assert m.uids[U[5]] == (1, 3) and m.uids[U[0]] == (0, 0) and m.next == [3, 4]


def test_model_register_moves_the_marks_and_refuses_a_created_uid():
    m = A.NodeModel(n_keys=16, R=2)
    m.register([U[0], U[1]], [0, 1], [7, 40])
    assert m.next == [8, 41]  # one past the largest, not the count
    st, idx = m.create_uids([U[0], U[2], U[3]], [0, 0, 1])
    assert st == [A.EXISTS, A.CREATED, A.CREATED] and idx == [7, 8, 41]
    with pytest.raises(A.Refused) as e:
        m.register([U[2]], [0], [3])
    assert e.value.code == A.EINVAL
    m.register([U[4]], [0], [2])  # a row below the mark leaves it
    assert m.next == [9, 42]


def test_model_store_growth_and_refusals_change_nothing():
    m = A.NodeModel(n_keys=4, R=2)
    m.create_uids(U[:10], [0] * 10, replica=[REP] * 10, max_keys=64)
    assert m.n_keys == 10 and m.next == [10, 0] and all(m.cols[r] == [REP] for r in range(10))
    m.create_uids(U[10:11], [0], max_keys=64)
    assert m.n_keys == 20  # max(11, 2 x 10)
    m.create_uids(U[11:12], [0], max_keys=64)
    assert m.n_keys == 20
    before = (dict(m.uids), list(m.next), m.n_keys)
    big = [(1000 + k, 5) for k in range(60)]
    with pytest.raises(A.Refused) as e:
        m.create_uids(big, [0] * 60, max_keys=64)  # 12 + 60 > 64
    assert e.value.code == A.ESTATE and (m.uids, m.next, m.n_keys) == before
    with pytest.raises(A.Refused) as e:
        m.create_uids(big[:9], [0] * 9, max_keys=0)  # no room and the store may not grow
    assert e.value.code == A.ESTATE and (m.uids, m.next, m.n_keys) == before
    m.create_uids(big[:8] + big[:8], [0] * 16, max_keys=0)  # exactly fits: the repeats take no row
    assert m.next == [20, 0] and m.n_keys == 20
    for bad in ([(0, 0)], [U[0], (0, 0)]):
        with pytest.raises(A.Refused) as e:
            m.create_uids(bad, [0] * len(bad))
        assert e.value.code == A.EINVAL
    with pytest.raises(A.Refused):
        A.NodeModel(n_keys=0, R=0).create_uids(U[:1], [0])  # no PN-Counter store
    with pytest.raises(A.Refused):
        A.NodeModel(n_keys=4, R=1, has_orset=False).create_uids(U[:1], [1])


def test_model_adoption():
    pro, stb = A.NodeModel(n_keys=8, R=2), A.NodeModel(n_keys=8, R=2)
    pro.create_uids([U[0], U[1], U[2]], [0, 1, 0])
    stb.register([U[2]], [0], [5])
    journal = [(b"a", U[0], 0), (b"raw", (0, 0), 1), (b"b", U[3], 0), (b"c", U[2], 0), (b"d", U[1], 0), (b"e", U[0], 0), (b"bad", (0, 0), 2),
               (None, (0, 0), 3), (b"zero", (0, 0), 0)]
    st, kind, idx = stb.adopt(pro, journal, replica=[REP] * len(journal))
    assert st == [A.ADOPTED, A.SKIPPED, A.NO_TYPE, A.HAVE, A.ADOPTED, A.HAVE, A.SKIPPED, A.SKIPPED, A.NO_TYPE]
    assert kind == [0, 255, 255, 0, 1, 0, 255, 255, 255]
    assert idx == [6, A.NO_IDX, A.NO_IDX, 5, 0, 6, A.NO_IDX, A.NO_IDX, A.NO_IDX]
    assert stb.cols == {6: [REP]} and stb.next == [7, 1]
    # the missing uid is created on the prospective copy: the same range again adopts it and nothing else
    pro.create_uids([U[3]], [1])
    st, kind, idx = stb.adopt(pro, journal)
    assert st == [A.HAVE, A.SKIPPED, A.ADOPTED, A.HAVE, A.HAVE, A.HAVE, A.SKIPPED, A.SKIPPED, A.NO_TYPE]
    assert kind[2] == 1 and idx[2] == 1 and stb.next == [7, 2]
    stb.wave_open = True
    with pytest.raises(A.Refused) as e:
        stb.adopt(pro, journal)
    assert e.value.code == A.EINVAL
