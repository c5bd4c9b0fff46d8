"""GPU parity of the OR-Set by element name (jg_orset_*_names, csrc/orset_names.hip).

Every batch is checked three ways:
  * against ORSetStr, the transcription of ORSet<string> (tests/orset_names_ref.py): each op's result,
    contains_names, and lookup_all_names' content and order;
  * against a TWIN store driven by ids the way a caller with its own dictionaries drives it (Interner +
    jg_orset_names_sync + jg_orset_apply_ops_ords): read() with ords, the ord limits, encode_json's bytes and the
    names log must be identical;
  * resolve_names against the Interner's live map.
The names log must also list a batch's new names in the order of their first Add.
"""
import numpy as np
import pytest

import janus_gpu as jg
import jsongen as J
from orset_names_ref import ADD, CLEAR, NEVER, NULL_ELEM, REMOVE, Interner, ORSetStr

pytestmark = pytest.mark.gpu


class Pair:
    """A by-name store, its id-driven twin, the string model of every set and the id rule."""

    def __init__(self, ctx, seed=0):
        self.st, self.tw = jg.ORSetStore(ctx), jg.ORSetStore(ctx)
        self.model, self.it = {}, Interner()
        self.rng = np.random.default_rng(seed)
        self.vocab = {}  # set -> names ever used there (what resolve / contains are asked about)

    def close(self):
        self.st.close()
        self.tw.close()

    def tags(self, n):
        return self.rng.integers(1, 2**63, n, dtype=np.uint64), self.rng.integers(0, 2**63, n, dtype=np.uint64)

    def _sync_twin(self, events):
        """The twin is told what a mirroring caller would tell it: runs of new names, and each Clear on its own."""
        run = []

        def flush():
            if run:
                nx = {}
                for s, i, _ in run:
                    nx[s] = i + 1
                self.tw.names_sync(list(nx), list(nx.values()), [0] * len(nx), list(run))
                run.clear()

        nxt = {}
        for ev in events:
            if ev[0] == "name":
                run.append(ev[1:])
                nxt[ev[1]] = ev[2] + 1
            else:
                flush()
                self.tw.names_sync([ev[1]], [nxt.get(ev[1], self.it_next0.get(ev[1], 0))], [1], [])
        flush()

    def batch(self, ops, check=True):
        """ops: [(set, op, name | None)].  Returns (results, ids)."""
        n = len(ops)
        sets, opc, names = [o[0] for o in ops], [o[1] for o in ops], [o[2] for o in ops]
        lo, hi = self.tags(n)
        log0 = len(self.it.log)
        self.it_next0 = dict(self.it.next_id)
        exp_res, exp_ids, events = [], [], []
        for k, (s, op, name) in enumerate(ops):
            exp_res.append(1 if self.model.setdefault(s, ORSetStr()).apply(op, name, (int(lo[k]), int(hi[k]))) else 0)
            i, ev = self.it.op(s, op, name)
            exp_ids.append(i)
            if ev:
                events.append(ev)
            if op != CLEAR:
                self.vocab.setdefault(s, {}).setdefault(name)
        res, ids, al, rl = self.st.apply_ops_names(sets, names, opc, lo, hi, ords=True)
        self._sync_twin(events)
        r2, al2, rl2 = self.tw.apply_ops_ords(sets, exp_ids, opc, lo, hi)
        assert res.tolist() == exp_res == r2.tolist()
        assert ids.tolist() == exp_ids
        assert np.array_equal(al, al2) and np.array_equal(rl, rl2)
        end, log = self.st.names_since(0)
        assert log[log0:] == self.it.log[log0:]  # this batch's new names, in first-Add op order
        if check:
            self.check()
        return res, ids

    def check(self, extra_sets=()):
        st, tw = self.st, self.tw
        for a, b in zip(st.read(), tw.read()):
            assert np.array_equal(a, b)  # keys, tags and ords
        e1, l1 = st.names_since(0)
        e2, l2 = tw.names_since(0)
        assert e1 == e2 == len(self.it.log) and l1 == l2 == self.it.log
        sets = sorted(set(self.model) | set(extra_sets))
        if not sets:
            return
        assert st.encode_json(sets) == tw.encode_json(sets)
        qs, qn = [], []
        for s in sets:
            for name in list(self.vocab.get(s, {})) + [None, b"never-seen"]:
                qs.append(s)
                qn.append(name)
        assert st.resolve_names(qs, qn).tolist() == [self.it.id_of(s, x) for s, x in zip(qs, qn)]
        members = {s: self.model[s].LookupAll() if s in self.model else [] for s in sets}
        present = {s: set(m) for s, m in members.items()}  # Contains(item) is LookupAll().Contains(item), ORSet.cs:236
        assert st.contains_names(qs, qn).tolist() == [1 if x in present[s] else 0 for s, x in zip(qs, qn)]
        names, ids = st.lookup_all_names(sets, with_ids=True)
        assert names == [members[s] for s in sets]
        for a, b in zip(ids, st.lookup_all(sets)):
            assert np.array_equal(a, b)


@pytest.fixture
def pair(ctx):
    p = Pair(ctx)
    yield p
    p.close()


def test_kat_single_orset_reference_type(pair):
    """ORSetTests.cs:57-81 replayed by name, its asserts literally."""
    st = pair.st
    pair.batch([(0, ADD, b"1")])
    pair.batch([(0, ADD, b"2")])
    assert pair.batch([(0, REMOVE, b"1")])[0][0] == 1
    assert pair.batch([(0, REMOVE, b"3")])[0][0] == 0
    pair.batch([(0, ADD, b"3")])
    assert len(st.lookup_all_names([0])[0]) == 2
    assert sorted(st.lookup_all_names([0])[0]) == [b"2", b"3"]
    pair.batch([(0, CLEAR, None)])
    assert st.lookup_all_names([0])[0] == []
    assert st.contains_names([0], [b"1"])[0] == 0
    pair.batch([(0, ADD, b"1")])
    assert st.contains_names([0], [b"1"])[0] == 1


def test_kat_single_orset_reference_type2(pair):
    """ORSetTests.cs:85-100: the "" element after a Clear."""
    st = pair.st
    pair.batch([(0, ADD, b"1")])
    pair.batch([(0, ADD, b"1")])
    assert st.lookup_all_names([0])[0] == [b"1"]
    pair.batch([(0, CLEAR, None)])
    pair.batch([(0, ADD, b"")])
    assert st.contains_names([0], [b""])[0] == 1


def _random_ops(rng, n, n_sets=3, vocab=40):
    names = [b"e%d" % k for k in range(vocab)] + [None]
    ops = []
    for _ in range(n):
        u = rng.random()
        op = CLEAR if u < 0.02 else (ADD if u < 0.6 else REMOVE)
        ops.append((int(rng.integers(0, n_sets)), op, names[int(rng.integers(0, len(names)))]))
    return ops


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4097])
def test_batch_sizes(ctx, n):
    """A wave, a workgroup and one scan tile past; 3 sets over 40 names, so names repeat within waves.  Two batches:
    the second meets resident names."""
    p = Pair(ctx, seed=n)
    try:
        p.batch(_random_ops(p.rng, n))
        p.batch(_random_ops(p.rng, n))
    finally:
        p.close()


@pytest.mark.parametrize("n", [64, 4096])
def test_contention_one_new_name(pair, n):
    res, ids = pair.batch([(2, ADD, b"the same new name")] * n)
    assert ids.tolist() == [0] * n and res.tolist() == [1] * n
    assert pair.st.names_since(0)[1] == [(2, 0, b"the same new name")]


def test_same_name_in_three_sets(pair):
    """1500 is past the element table's first 1024 sets."""
    res, ids = pair.batch([(0, ADD, b"n"), (1, ADD, b"m"), (1, ADD, b"n"), (1500, ADD, b"n"), (0, ADD, b"n")])
    assert ids.tolist() == [0, 0, 1, 0, 0]
    assert pair.st.names_since(0)[1] == [(0, 0, b"n"), (1, 0, b"m"), (1, 1, b"n"), (1500, 0, b"n")]
    pair.check(extra_sets=[7, 4000])  # never-seen set ids are empty sets


def test_order_remove_then_add(pair):
    res, ids = pair.batch([(0, REMOVE, b"x"), (0, ADD, b"x")])
    assert res.tolist() == [0, 1] and ids.tolist() == [NEVER, 0]
    assert pair.st.contains_names([0], [b"x"])[0] == 1


def test_order_add_then_remove(pair):
    res, ids = pair.batch([(0, ADD, b"x"), (0, REMOVE, b"x")])
    assert res.tolist() == [1, 1] and ids.tolist() == [0, 0]
    assert pair.st.contains_names([0], [b"x"])[0] == 0


def test_order_add_clear_add(pair):
    pair.batch([(0, ADD, b"w")])
    res, ids = pair.batch([(0, ADD, b"x"), (0, CLEAR, None), (0, ADD, b"x")])
    assert ids.tolist() == [1, 0, 2]  # ids k and k + 1, both in the log
    assert pair.st.names_since(0)[1] == [(0, 0, b"w"), (0, 1, b"x"), (0, 2, b"x")]
    assert pair.st.contains_names([0], [b"x"])[0] == 1
    assert pair.st.lookup_all_names([0])[0] == [b"x"]
    assert pair.st.resolve_names([0, 0], [b"x", b"w"]).tolist() == [2, NEVER]


def test_order_resident_clear_remove(pair):
    pair.batch([(0, ADD, b"x"), (1, ADD, b"x")])
    res, ids = pair.batch([(0, CLEAR, None), (0, REMOVE, b"x"), (1, REMOVE, b"x")])
    assert res.tolist() == [1, 0, 1] and ids.tolist() == [0, NEVER, 0]


def test_null_and_empty(pair):
    res, ids = pair.batch([(0, ADD, None), (0, REMOVE, None), (0, REMOVE, None), (0, ADD, b""), (0, ADD, None)])
    assert res.tolist() == [1, 1, 0, 1, 1] and ids.tolist() == [NULL_ELEM, NULL_ELEM, NULL_ELEM, 0, NULL_ELEM]
    assert pair.st.lookup_all_names([0])[0] == [b"", None]


_LENS = [0, 1, 7, 8, 9, 15, 16, 17, 255, 256, 4096]


def _byte_names():
    base = bytes((37 * k + 11) % 251 + 1 for k in range(4096))
    names = [base[:n] for n in _LENS]                       # prefixes of each other, every length
    names += [base[:n - 1] + b"\xff" for n in _LENS if n]   # differing only in the last byte
    names += [b"a\x00b", b"a\x00", b"a", b"\x00", "żółć".encode(), "名前".encode(), "🙂".encode(), "🙂🙂".encode()]
    assert len(set(names)) == len(names)
    return names


@pytest.mark.parametrize("bits", [None, "3"])
def test_bytes(ctx, bits, monkeypatch):
    """Name lengths around the 8- and 16-byte steps and the pool's alignment, prefixes, last-byte differences, an
    embedded 0x00, multi-byte UTF-8; again with 3-bit name hashes, where the byte compare decides every probe."""
    if bits:
        monkeypatch.setenv("JANUS_TEST_NAME_HASH_BITS", bits)
    p = Pair(ctx, seed=5)
    try:
        names = _byte_names()
        ops = [(k % 2, ADD, x) for k, x in enumerate(names)] + [(1 - k % 2, REMOVE, x) for k, x in enumerate(names)]
        ops += [(k % 2, ADD, x) for k, x in enumerate(names)]  # the batch's own names, found again
        p.batch(ops)
        p.batch([(k % 2, REMOVE, x) for k, x in enumerate(names[::2])] + [(1 - k % 2, ADD, x) for k, x in enumerate(names)])
    finally:
        p.close()


def test_growth_names(pair):
    """One batch past the 4,096-name first allocation (a table rebuild): all 5,000 then resolve."""
    names = [b"name-%d" % k for k in range(5000)]
    pair.batch([(0, ADD, b"before")])
    res, ids = pair.batch([(0, ADD, x) for x in names], check=False)
    assert ids.tolist() == list(range(1, 5001))
    assert pair.st.resolve_names([0] * 5001, names + [b"before"]).tolist() == list(range(1, 5001)) + [0]
    pair.check()


def test_growth_pool(pair):
    """300 names of 4 KB: past the 1 MiB first pool."""
    names = [(b"%04d" % k) * 1024 for k in range(300)]
    pair.batch([(3, ADD, b"before")])
    pair.batch([(3, ADD, x) for x in names], check=False)
    assert pair.st.resolve_names([3] * 301, names + [b"before"]).tolist() == list(range(1, 301)) + [0]
    assert pair.st.lookup_all_names([3])[0] == [b"before"] + names


def test_mixing_names_sync(pair):
    """Names registered by jg_orset_names_sync resolve by name; after its Clear the old names no longer do."""
    for st in (pair.st, pair.tw):
        st.names_sync([4], [2], [0], [(4, 0, b"p"), (4, 1, b"q")])
    pair.it.adopt(4, 0, b"p")
    pair.it.adopt(4, 1, b"q")
    assert pair.st.resolve_names([4, 4, 4], [b"p", b"q", b"r"]).tolist() == [0, 1, NEVER]
    res, ids = pair.batch([(4, ADD, b"q"), (4, ADD, b"r"), (4, REMOVE, b"p")])
    assert ids.tolist() == [1, 2, 0] and res.tolist() == [1, 1, 0]
    for st in (pair.st, pair.tw):
        st.names_sync([4], [3], [1], [])
    pair.it.clear(4)
    assert pair.st.resolve_names([4, 4, 4], [b"p", b"q", b"r"]).tolist() == [NEVER] * 3
    assert pair.batch([(4, ADD, b"q")], check=False)[1].tolist() == [3]


def test_mixing_waves(pair):
    """A wave's names are found by name, unescaped; a wave after a by-name batch reuses the batch's ids."""
    g = J.random_guids(pair.rng, 3)
    msg = ('{"addSet":{"a\\u0041":["%s"]},"removeSet":{},"nullAddGuid":[],"nullRemoveGuid":[]}' % J.guid_d(*g[0])).encode()
    pair.st.merge_json([6], [msg])
    assert pair.st.wave_names() == [(6, 0, b"aA")]
    assert pair.st.resolve_names([6, 6], [b"aA", b"a\\u0041"]).tolist() == [0, NEVER]
    assert pair.st.contains_names([6], [b"aA"])[0] == 1
    assert pair.st.lookup_all_names([6])[0] == [b"aA"]
    res, ids = pair.st.apply_ops_names([6, 6], [b"aA", b"zz"], [ADD, ADD], *pair.tags(2))
    assert ids.tolist() == [0, 1]
    pair.st.merge_json([6], [J.encode_orset([("zz", [g[1]]), ("aA", [g[2]]), ("new", [g[1]])], [])])
    assert pair.st.wave_names() == [(6, 2, b"new")]  # nothing issued again for the batch's strings
    assert pair.st.lookup_all_names([6])[0] == [b"aA", b"zz", b"new"]


def test_lookup_all_names_buffers(pair):
    pair.batch([(0, ADD, b"alpha"), (0, ADD, b""), (0, ADD, None), (2, ADD, b"beta"), (2, ADD, b"gamma"), (2, REMOVE, b"beta")])
    st, lib = pair.st, jg.load()
    sets = np.array([0, 1, 2, 999999], np.uint32)  # 1: empty, 999999: never seen
    assert st.lookup_all_names(sets) == [[b"alpha", b"", None], [], [b"gamma"], []]
    off, nb = np.zeros(5, np.uint64), jg.C.c_uint64()
    p = lambda a: a.ctypes.data_as(jg.C.c_void_p)  # noqa: E731
    assert lib.jg_orset_lookup_all_names(st._h, 4, p(sets), p(off), jg.C.byref(nb), None, None, None, None, 0, 0) == jg.JG_OK
    assert off.tolist() == [0, 3, 3, 4, 4] and nb.value == 10

    def call(cap_e, cap_b):
        noff, data = np.full(5, 77, np.uint64), np.full(10, 77, np.uint8)
        isn, ids = np.full(4, 77, np.uint8), np.full(4, 77, np.uint32)
        rc = lib.jg_orset_lookup_all_names(st._h, 4, p(sets), p(off), jg.C.byref(nb), p(noff), p(data), p(isn), p(ids), cap_e, cap_b)
        return rc, noff, data, isn, ids

    rc, noff, data, isn, ids = call(4, 10)  # an exact fit
    assert rc == jg.JG_OK and noff.tolist() == [0, 5, 5, 5, 10] and data.tobytes() == b"alphagamma"
    assert isn.tolist() == [0, 0, 1, 0] and ids.tolist() == [0, 1, NULL_ELEM, 1]
    for caps in ((3, 10), (4, 9)):  # one element, one byte short: nothing written
        rc, noff, data, isn, ids = call(*caps)
        assert rc == jg.JG_ESTATE
        assert set(noff.tolist()) | set(data.tolist()) | set(isn.tolist()) | set(ids.tolist()) == {77}


def test_refusals(pair):
    pair.batch([(0, ADD, b"x")])
    st = pair.st
    before = (st.size(), st.names_since(0), st.resolve_names([0, 0], [b"x", b"y"]).tolist())
    with pytest.raises(jg.JanusError) as e:
        st.apply_ops_names([0, 0], [b"y", b"z"], [ADD, 4], *pair.tags(2))
    assert e.value.code == jg.JG_EINVAL
    assert (st.size(), st.names_since(0), st.resolve_names([0, 0], [b"x", b"y"]).tolist()) == before
    jg._check(jg.load().jg_orset_wave_begin(st._h, 1, 16))
    try:
        with pytest.raises(jg.JanusError) as e:
            st.apply_ops_names([0], [b"y"], [ADD], *pair.tags(1))
        assert e.value.code == jg.JG_EINVAL
        assert st.contains_names([0], [b"x"])[0] == 1  # the read-only calls go on, as jg_orset_contains does
    finally:
        jg._check(jg.load().jg_orset_wave_abort(st._h))
    assert (st.size(), st.names_since(0), st.resolve_names([0, 0], [b"x", b"y"]).tolist()) == before
