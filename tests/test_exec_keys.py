"""CPU-only: the surface of the client batches by key name (jg_node_exec_keys): both libraries export the
symbol, the binding's signature has one entry per parameter the header declares, pack_exec on a hand-made batch, and
the sequential model the GPU tests hold the call to (exec_keys_ref.ExecModel) on hand-worked cases."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import janus_gpu as jg
from exec_keys_ref import (INC, DEC, NO_IDX, Q_NO_ARG, Q_NO_CRDT, Q_NO_KEY, Q_OK, Q_OVERFLOW, U_BAD_ARG, U_BAD_OP, U_NO_KEY, U_OK,
                           ExecModel)
from orset_names_ref import ADD, CLEAR, NEVER, NULL_ELEM, REMOVE

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "janus_gpu.h").read_text()
EXEC, SHIP = "jg_node_exec_keys", "jg_node_update_keys_ship"
NA = jg.NULL_ARG


def declaration(name):
    return [p.strip() for p in re.search(r"^int %s\((.*?)\);" % name, HEADER, flags=re.M | re.S).group(1).split(",")]


def test_both_libraries_export_the_symbol():
    for path in (jg.LIB_PATH, jg.LIB_PATH.with_name("libjanusgpu_test.so")):
        assert hasattr(ctypes.CDLL(str(path)), EXEC), path
    assert EXEC in jg.EXPORTS


def test_signature_has_one_entry_per_header_parameter():
    """jg_node_update_keys_ship's parameters with cmd behind key_bytes and value behind result: 28."""
    params, ship = declaration(EXEC), declaration(SHIP)
    assert len(params) == 28
    assert params[5] == "const uint8_t* cmd" and params[17] == "int64_t* value"
    assert [p for i, p in enumerate(params) if i not in (5, 17)] == ship
    args, res = jg._SIGS[EXEC]
    assert len(args) == 28 and res is ctypes.c_int
    assert args[2] is ctypes.c_uint64 and args[13] is ctypes.c_uint32 and args[25] is ctypes.c_uint64
    assert all(a is ctypes.c_void_p for i, a in enumerate(args) if i not in (2, 13, 25))


def test_the_header_states_the_rules():
    doc = HEADER[HEADER.index("Client batches by key name"):HEADER.index("int %s(" % EXEC)]
    for text in ("additive to ABI v10", "PNCWorkload.cs:44-59", "ORSetWorkload.cs:66-138", "QueryProspective", "JG_Q_OVERFLOW", "JG_Q_NO_ARG",
                 "cmd[i] above 1", "a read with arg_flag 3", "refused while a wave holds a store", "jg_node_shipped", "never opens or cuts a round",
                 "interns nothing"):
        assert text in doc, text


def test_the_wrapper_takes_what_the_issue_names():
    sig = inspect.signature(jg.Node.exec_keys)
    assert list(sig.parameters)[1:] == ["keyspace", "keys", "cmds", "ops", "args", "snap", "tags", "col", "sha", "cap", "with_guid"]
    p = sig.parameters
    assert p["snap"].default is None and p["tags"].default is None and p["col"].default == 0 and p["sha"].default is False
    assert p["cap"].default is None and p["with_guid"].default is False


def test_packing_of_a_hand_made_batch():
    keys = [b"k", "ab", b"", b"k"]
    koff, kdata, cmd, op, flag, amount, eoff, edata = jg.pack_exec(keys, [0, 1, 1, 0], [1, None, 2, 3], [7, "x", NA, None])
    assert koff.tolist() == [0, 1, 3, 3, 4] and kdata.tobytes() == b"kabk"
    assert cmd.dtype == np.uint8 and cmd.tolist() == [0, 1, 1, 0]
    assert op.dtype == np.uint8 and op.tolist() == [1, 0, 2, 3]
    assert flag.tolist() == [3, 1, 2, 0]
    assert amount.dtype == np.int64 and amount.tolist() == [7, 0, 0, 0]
    assert eoff.tolist() == [0, 0, 1, 1, 1] and edata.tobytes() == b"x"


def test_packing_of_reads_only_and_its_refusals():
    koff, kdata, cmd, op, flag, amount, eoff, edata = jg.pack_exec([b"a", b"b"], [1, 1], None, [None, ""])
    assert op is None and amount is None and cmd.tolist() == [1, 1] and flag.tolist() == [0, 1]
    assert eoff.tolist() == [0, 0, 0] and edata.size == 1  # "" is a string: both element pointers are given
    *_, amount, eoff, edata = jg.pack_exec([b"a"], [1], None, [None])
    assert amount is None and eoff is None and edata is None
    *_, amount, _, _ = jg.pack_exec([b"a"], [1], [0], [5])  # an integer on a read is packed as flag 3 and left to the library to refuse
    assert amount is None
    with pytest.raises(ValueError):
        jg.pack_exec([b"a"], [0], None, [1])
    with pytest.raises(ValueError):
        jg.pack_exec([b"a", b"b"], [0], [1, 1], [1, 1])


# ---- the sequential model on hand-worked cases ------------------------------------------------------------------------
G = [(i + 1, 100 + i) for i in range(4)]


def world(eb, P0=None):
    guid = {b"p": G[0], b"s": G[1], b"lost": G[2]}
    reg = {G[0]: (0, 1), G[1]: (1, 7)}
    dt = np.int32 if eb == 4 else np.int64
    P, N = np.zeros((2, 4), dt), np.zeros((2, 4), dt)
    if P0 is not None:
        P[1] = P0
    return ExecModel(guid, reg, P, N, null=NA)


def tags(n):
    return np.arange(1, n + 1, dtype=np.uint64), np.zeros(n, np.uint64)


@pytest.mark.parametrize("eb", [4, 8])
def test_model_overflow_appears_and_disappears_within_a_batch(eb):
    top = 2**31 - 1 if eb == 4 else 2**63 - 1
    m = world(eb, [top, 0, 0, 0])
    out = m.run([(b"p", True, 0, None), (b"p", False, INC, 1), (b"p", True, 0, None)], *tags(3), col=2)
    assert out["status"].tolist() == [Q_OK, U_OK, Q_OVERFLOW] and out["value"].tolist() == [top, 0, 0]
    assert m.P[1].tolist() == [top, 0, 1, 0]  # the write is applied either way
    out = m.run([(b"p", True, 0, None), (b"p", False, INC, -1), (b"p", True, 0, "ignored")], *tags(3), col=2)
    assert out["status"].tolist() == [Q_OVERFLOW, U_OK, Q_OK] and out["value"].tolist() == [0, 0, top]
    assert out["result"].tolist() == [0, 1, 0] and out["idx"].tolist() == [1, 1, 1] and out["kind"].tolist() == [0, 0, 0]


def test_model_counter_reads_see_exactly_the_writes_before_them():
    m = world(4)
    cmds = [(b"p", True, 0, None), (b"p", False, INC, 5), (b"p", True, 0, None), (b"p", False, DEC, 7), (b"p", True, 0, None),
            (b"p", False, INC, 2**31), (b"p", True, 0, None)]  # 5 + 2^31 wraps the int32 cell to 5 - 2^31
    out = m.run(cmds, *tags(7), col=0)
    # (5 - 2^31) - 7 leaves int32, but Get's '-' is unchecked and wraps; only Sum's '+' is checked, and both sums fit
    assert out["value"].tolist() == [0, 0, 5, 0, -2, 0, 2**31 - 2]
    assert out["status"].tolist() == [Q_OK, U_OK, Q_OK, U_OK, Q_OK, U_OK, Q_OK]
    assert m.P[1, 0] == 5 - 2**31 and m.N[1, 0] == 7


def test_model_one_name_through_add_remove_clear_add():
    m = world(8)
    cmds = [(b"s", False, ADD, "x"), (b"s", True, 0, "x"), (b"s", False, REMOVE, "x"), (b"s", True, 0, "x"), (b"s", False, ADD, "x"),
            (b"s", True, 0, "x"), (b"s", False, CLEAR, None), (b"s", True, 0, "x"), (b"s", False, ADD, "x"), (b"s", True, 0, "x"),
            (b"s", True, 0, "y"), (b"s", True, 0, NA), (b"s", True, 0, None)]
    out = m.run(cmds, *tags(len(cmds)))
    assert out["value"].tolist() == [0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
    assert out["status"].tolist() == [U_OK, Q_OK] * 5 + [Q_OK, Q_OK, Q_NO_ARG]
    assert out["result"].tolist() == [1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0]
    # the name keeps id 0 until the Clear drops it; the Add after the Clear is issued id 1; "y" was never held
    assert out["elem"].tolist() == [0, 0, 0, 0, 0, 0, 0, NEVER, 1, 1, NEVER, NULL_ELEM, NEVER]
    assert out["idx"].tolist() == [7] * 12 + [NO_IDX]
    assert m.it.log == [(7, 0, b"x"), (7, 1, b"x")]


def test_model_membership_follows_the_tags_not_the_last_op():
    """Add(t1), Remove, Add(t1) again: the tag is already tombstoned, the sets of tags are equal, the element stays absent."""
    m = world(8)
    lo, hi = np.array([9, 0, 0, 9, 0], np.uint64), np.zeros(5, np.uint64)
    out = m.run([(b"s", False, ADD, "x"), (b"s", False, REMOVE, "x"), (b"s", True, 0, "x"), (b"s", False, ADD, "x"), (b"s", True, 0, "x")], lo, hi)
    assert out["value"].tolist() == [0, 0, 0, 0, 0] and out["result"].tolist() == [1, 1, 0, 1, 0]


def test_model_statuses_of_both_kinds():
    m = world(8)
    cmds = [(b"none", True, 0, None), (b"none", False, INC, 1), (b"lost", True, 0, None), (b"lost", False, ADD, "x"), (b"p", False, INC, "x"),
            (b"p", False, 9, 1), (b"s", False, 4, "x"), (b"s", False, ADD, 3), (b"s", True, 0, 3)]
    out = m.run(cmds, *tags(len(cmds)))
    assert out["status"].tolist() == [Q_NO_KEY, U_NO_KEY, Q_NO_CRDT, 2, U_BAD_ARG, U_BAD_OP, U_BAD_OP, U_BAD_ARG, Q_NO_ARG]
    assert out["kind"].tolist() == [255, 255, 255, 255, 0, 0, 1, 1, 1]
    assert (out["idx"] == NO_IDX).all() and (out["elem"] == NEVER).all() and not out["value"].any() and not out["result"].any()
    assert out["guid"]["lo"].tolist() == [0, 0, 3, 3, 1, 1, 2, 2, 2]
