"""CPU-only: the by-name OR-Set surface (jg_orset_*_names) is declared, bound and exported, and the two test-only
restatements the GPU tests compare against (tests/orset_names_ref.py) reproduce the reference's own known answers
(MergeSharp/MergeSharp.Tests/ORSetTests.cs) and hand-worked cases of the id rule."""
import ctypes

import janus_gpu as jg
from orset_names_ref import ADD, CLEAR, NEVER, NULL_ELEM, REMOVE, Interner, ORSetStr

NAMES = ["jg_orset_resolve_names", "jg_orset_contains_names", "jg_orset_lookup_all_names", "jg_orset_apply_ops_names"]


def test_entry_points_bound_and_exported():
    lib = ctypes.CDLL(str(jg.LIB_PATH))
    for name in NAMES:
        assert name in jg.EXPORTS, name
        assert hasattr(lib, name), name
    assert lib.jg_abi_version() == 10  # additive, as the key-space functions were
    for m in ("resolve_names", "contains_names", "lookup_all_names", "apply_ops_names"):
        assert callable(getattr(jg.ORSetStore, m))


def test_single_orset_reference_type():
    """ORSetTests.cs:57-81, its asserts literally."""
    s, t = ORSetStr(), iter(range(100))
    s.Add(b"1", next(t))
    s.Add(b"2", next(t))
    assert s.Remove(b"1") is True
    assert s.Remove(b"3") is False
    s.Add(b"3", next(t))
    assert s.Count == 2
    assert sorted(s.LookupAll()) == [b"2", b"3"]
    s.Clear()
    assert s.Count == 0
    assert s.LookupAll() == []
    assert s.Contains(b"1") is False
    s.Add(b"1", next(t))
    assert s.Contains(b"1") is True


def test_single_orset_reference_type2():
    """ORSetTests.cs:85-100: the "" element after a Clear."""
    s = ORSetStr()
    s.Add(b"1", 1)
    s.Add(b"1", 2)
    assert s.Count == 1
    assert s.LookupAll() == [b"1"]
    s.Clear()
    s.Add(b"", 3)
    assert s.Contains(b"") is True


def test_lookup_all_order_and_null():
    s = ORSetStr()
    for k, n in enumerate([b"a", b"b", b"c", None]):
        s.Add(n, k)
    assert s.Remove(b"a") and s.Remove(None)
    s.Add(b"a", 10)  # a: tag sets differ again, b and c have no tombstones
    assert s.LookupAll() == [b"b", b"c", b"a"]  # only-in-add first, then differing tag sets
    s.Add(None, 11)
    assert s.LookupAll() == [b"b", b"c", b"a", None]
    assert s.Remove(None) and not s.Remove(None)


def test_interner_remove_before_first_add():
    it = Interner()
    assert it.op(0, REMOVE, b"x") == (NEVER, None)  # nothing interned, also though an Add follows
    assert it.op(0, ADD, b"x") == (0, ("name", 0, 0, b"x"))
    assert it.op(0, REMOVE, b"x") == (0, None)
    assert it.op(0, ADD, b"x") == (0, None)
    assert it.log == [(0, 0, b"x")]


def test_interner_add_clear_add_gives_two_ids():
    it = Interner()
    assert it.op(5, ADD, b"x")[0] == 0
    assert it.op(5, ADD, b"y")[0] == 1
    assert it.op(5, CLEAR, None) == (0, ("clear", 5))
    assert it.op(5, REMOVE, b"x") == (NEVER, None)  # dead after the Clear
    assert it.op(5, ADD, b"x")[0] == 2              # ids only grow, also across Clear
    assert it.log == [(5, 0, b"x"), (5, 1, b"y"), (5, 2, b"x")]
    assert it.id_of(5, b"x") == 2 and it.id_of(5, b"y") == NEVER and it.id_of(5, None) == NULL_ELEM


def test_interner_same_name_in_two_sets():
    it = Interner()
    assert it.op(0, ADD, b"n")[0] == 0
    assert it.op(1, ADD, b"m")[0] == 0
    assert it.op(1, ADD, b"n")[0] == 1
    assert it.op(0, ADD, None) == (NULL_ELEM, None)
    assert it.log == [(0, 0, b"n"), (1, 0, b"m"), (1, 1, b"n")]
    assert it.id_of(7, b"n") == NEVER  # a set never seen is empty
