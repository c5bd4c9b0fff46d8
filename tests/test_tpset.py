"""CPU-only: the restatement of TPSet<string> (tests/tpset_ref.py) against the reference's known answers
(MergeSharp.Tests/2PSetTests.cs) and the wire form its encoder writes."""
import tpset_ref as R


def _set(*adds):
    s = R.TPSetRef()
    for x in adds:
        s.add(x)
    return s


def test_tpset_single():  # TestTPsetSingle
    s = _set(b"a", b"b")
    assert s.remove(b"a")
    assert not s.remove(b"c")  # this remove should have no effect
    s.add(b"c")
    assert s.count() == 2
    assert s.lookup_all() == [b"b", b"c"]


def _set2():
    s2 = _set(b"c", b"d")
    s2.remove(b"c")
    return s2


def test_tpset_merge():  # TestTPsetMerge
    s, s2 = _set(b"a", b"b"), _set2()
    s.merge(list(s2.add_set), list(s2.rem_set))
    assert s.lookup_all() == [b"a", b"b", b"d"]


def test_true_equals():  # TrueEquals: LookupAll().SequenceEqual
    assert _set(b"a", b"b").lookup_all() == _set(b"a", b"b").lookup_all()


def test_false_equals():  # FalseEquals
    assert _set(b"a", b"b").lookup_all() != _set(b"c").lookup_all()


def test_encode_decode():  # TPSetMsgTests.EncodeDecode
    s, s2 = _set(b"a", b"b"), _set2()
    wire = s2.encode()
    assert wire == b'{"addSet":["c","d"],"removeSet":["c"]}'
    assert s.merge_json([wire]) == (None, False)
    assert s.lookup_all() == [b"a", b"b", b"d"]


def test_key_space_entry_encoding():
    """KeySpaceManager's entries are key + "\\0" + guid: NUL goes out as \\u0000 (JavaScriptEncoder.Default)."""
    assert R.encode_msg([b"k\0g"], []) == b'{"addSet":["k\\u0000g"],"removeSet":[]}'
    assert R.escape(b'"\\+\x7f\n') == b'\\u0022\\\\\\u002B\\u007F\\n'
    assert R.escape("é€😀".encode()) == b"\\u00E9\\u20AC\\uD83D\\uDE00"
    assert R.encode_msg([None, b""], [None]) == b'{"addSet":[null,""],"removeSet":[null]}'


def test_decode_contract():
    s = R.TPSetRef()
    msgs = [b' {"x":{"y":[1,2.5e3,true,null]}, "removeSet" : [ "b" ] ,"addSet":["a","a",null,"\\u0061"], "addSet":["z","\\uD83D\\uDE00"]} ',
            b'{"addSet":["p"]}', b'{"addSet":["never"],"removeSet":[]}']
    assert s.merge_json(msgs) == (1, True)
    assert list(s.add_set) == [b"z", "😀".encode(), b"p"] and list(s.rem_set) == [b"b"]
    for bad in (b'{"addSet":["a],"removeSet":[]}', b'{"addSet":["\\"],"removeSet":[]}', b'{"addSet":["\\u12G4"],"removeSet":[]}',
                b'{"addSet":["\\uD800"],"removeSet":[]}', b'{"addSet":["\xc0\x80"],"removeSet":[]}', b'{"addSet":["a" "b"],"removeSet":[]}',
                b'{"addSet":["a",],"removeSet":[]}', b'{"addSet":[["a"]],"removeSet":[]}', b'{"addSet":[1],"removeSet":[]}',
                b'{"addSet":["a"],"removeSet":[', b'{"removeSet":[]}', b'{"addSet":null,"removeSet":[]}'):
        t = R.TPSetRef()
        assert t.merge_json([bad]) == (0, False), bad
        assert t.size() == (0, 0, 0)
    deep = b'{"x":' + b"[" * 63 + b"]" * 63 + b',"addSet":[],"removeSet":[]}'
    assert R.TPSetRef().merge_json([deep]) == (None, False)
    deeper = b'{"x":' + b"[" * 64 + b"]" * 64 + b',"addSet":[],"removeSet":[]}'
    assert R.TPSetRef().merge_json([deeper]) == (0, False)


def test_binding_names_the_set():
    """The binding lists the key-space set's entry points (the ABI tests check them against the header and the
    library's exports)."""
    import janus_gpu as jg
    for name in ("jg_tpset_create", "jg_tpset_destroy", "jg_tpset_size", "jg_tpset_apply_ops", "jg_tpset_contains", "jg_tpset_lookup_all",
                 "jg_tpset_merge_json", "jg_tpset_encode_json", "jg_tpset_last_stats"):
        assert name in jg.EXPORTS
    import ctypes
    assert ctypes.sizeof(jg.TPSetStats) == 80


def _random_message(rng, pool):
    """A TPSetMsg in one of many spellings, sometimes broken or without a member."""
    def spell(x):
        if x is None:
            return b"null"
        o = b""
        for ch in x.decode():
            how = int(rng.integers(0, 3))
            o += ch.encode() if how == 0 and ord(ch) >= 0x20 and ch not in '"\\' else R.escape(ch.encode()) if how == 1 else \
                b"".join(b"\\u%04x" % u for u in ([ord(ch)] if ord(ch) < 0x10000 else
                                                  [0xD800 | (ord(ch) - 0x10000) >> 10, 0xDC00 | (ord(ch) - 0x10000) & 0x3FF]))
        return b'"' + o + b'"'
    pick = lambda k: [pool[i] for i in rng.integers(0, len(pool), k)]
    arr = lambda: b"[ " + b" ,".join(spell(x) for x in pick(int(rng.integers(0, 6)))) + b"]"
    members = [b'"addSet":' + arr(), b'"removeSet" : ' + arr(), b'"other":{"a":[1,2.5,null,"x"]}']
    form = int(rng.integers(0, 8))
    if form == 0:
        members = members[:1]  # no removeSet: partial
    elif form == 1:
        members = members[1:]  # no addSet
    elif form == 2:
        members.append(b'"addSet":null')
    elif form == 3:
        members.append(b'"addSet":' + arr())  # the last occurrence wins
    order = rng.permutation(len(members)) if form >= 4 else range(len(members))
    msg = b"{" + b",".join(members[i] for i in order) + b"} "
    return msg[: int(rng.integers(1, len(msg)))] if form == 7 else msg


def test_cpp_restatement_agrees_byte_for_byte():
    """host/tpset_ref.hpp (the C++ restatement, built as build/tpset_ref_dump) and tests/tpset_ref.py give the same
    Remove results, merge verdicts (the decoder and Merge, on many spellings and on malformed messages), Count,
    LookupAll size and encoded bytes on 300 random states over every escape class."""
    import subprocess
    from pathlib import Path

    import numpy as np
    exe = Path(__file__).resolve().parents[1] / "janus-crdt_amd" / "build" / "tpset_ref_dump"
    assert exe.exists(), "built by __graft_entry__.build()"
    rng = np.random.default_rng(17)
    alphabet = [b"\0", b'"', b"\\", b"+", b"\x7f", b"\n", b"\b", b"&", "é".encode(), "€".encode(), "😀".encode(), b"a", b"z", b"/"]
    script, expect = [], []
    for _ in range(300):
        pool = [b"", None] + [b"".join(alphabet[i] for i in rng.integers(0, len(alphabet), int(rng.integers(1, 5)))) for _ in range(12)]
        ref = R.TPSetRef()
        for _ in range(int(rng.integers(0, 40))):
            x = pool[int(rng.integers(0, len(pool)))]
            hx = "-" if x is None else x.hex()
            kind = int(rng.integers(0, 4))
            if kind == 3:
                msg = _random_message(rng, pool)
                bad, partial = ref.merge_json([msg])
                expect.append("0" if bad is None else "2" if partial else "1")
                script.append("M " + msg.hex())
            elif kind:
                ref.add(x)
                script.append("A " + hx)
            else:
                expect.append("1" if ref.remove(x) else "0")
                script.append("R " + hx)
        script.append("E")
        expect.append("%s %d %d" % (ref.encode().hex(), ref.count(), len(ref.lookup_all())))
    out = subprocess.run([str(exe)], input="\n".join(script) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split("\n")[:-1] == expect


def test_cpp_key_space_restatement_agrees():
    """host/tpset_ref.hpp's KeySpace (CreateNewKVPair, Receive = Merge + OnNext in the reference's order, ContainsKey
    before Guid.Parse, with the documented departure for malformed entries of unknown keys) and
    tests/tpset_ref.py's KeySpaceRef give the same verdicts, TryAdd results, journals and sets on random histories with
    repeated keys, removals, upper-case guids, malformed entries, the null element and rejected messages."""
    import subprocess
    from pathlib import Path

    import numpy as np
    exe = Path(__file__).resolve().parents[1] / "janus-crdt_amd" / "build" / "tpset_ref_dump"
    assert exe.exists(), "built by __graft_entry__.build()"
    rng = np.random.default_rng(23)
    guids = [(int(rng.integers(1, 1 << 62)), int(rng.integers(1, 1 << 62))) for _ in range(12)]
    keys = [b"k%d" % i for i in range(10)] + [b"", "ключ".encode()]
    script, expect = [], []
    for _ in range(120):
        ref = R.KeySpaceRef()
        for _ in range(int(rng.integers(1, 10))):
            k, g = keys[int(rng.integers(0, len(keys)))], guids[int(rng.integers(0, len(guids)))]
            if rng.integers(0, 3) == 0:
                expect.append("1" if ref.create_keys([(k, g)])[0] else "0")
                script.append("C %s %d %d" % (k.hex() or "", g[0], g[1]))
                continue
            add = []
            for _ in range(int(rng.integers(0, 6))):
                kk, gg = keys[int(rng.integers(0, len(keys)))], guids[int(rng.integers(0, len(guids)))]
                d = R.guid_d(gg)
                add.append([kk + b"\0" + d, kk + b"\0" + d.upper(), kk + b"\0" + d + b"\0more", kk + d, kk + b"\0{" + d + b"}", None][int(rng.integers(0, 6))])
            old = [x for x in ref.set.add_set if x is not None]
            rem = [old[int(rng.integers(0, len(old)))]] if old and rng.integers(0, 2) else []
            form = int(rng.integers(0, 8))
            msg = R.encode_msg(add, rem + add[:1] if form == 0 else rem)
            if form == 1:
                msg = msg[:msg.index(b',"removeSet"')] + b"}"  # partial: no OnNext
            elif form == 2:
                msg = msg[:-3]
            bad, partial = ref.receive([msg])
            expect.append("0" if bad is None else "2" if partial else "1")
            script.append("V " + msg.hex())
        script.append("J")
        expect += ["%d %s %d %d" % (st, b.hex(), g[0], g[1]) for b, g, st in ref.journal] + [ref.set.encode().hex()]
    out = subprocess.run([str(exe)], input="\n".join(script) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split("\n")[:-1] == expect


# ---- OnNext's order (KeySpaceManager.cs:160-172): ContainsKey(item.Split("\0")[0]) comes before Split(...)[1] and
# Guid.Parse, so an entry of a key the dictionary holds is skipped whatever the rest of it looks like.  Each case is
# (steps in the form test_keyspace_gpu.both() takes, the journal, the dictionary), the last two worked out by hand from
# those lines (with the stated departure: where the reference throws, a record with status 1 / 2 / 3 and no add).
_A, _B, _C, _D = (0x0123456789ABCDEF, 0x1122334455667788), (2, 3), (0xFFFFFFFFFFFFFFFF, 0), (0, 0)
_DA, _DB, _DC = b"89abcdef-4567-0123-8877-665544332211", b"00000002-0000-0000-0300-000000000000", b"ffffffff-ffff-ffff-0000-000000000000"
_OK = (None, False)


def _m(add, rem=()):
    return R.encode_msg(list(add), list(rem))


ORDER_CASES = {
    # both malformed entries are of known keys, and new\0zz comes after new was added: one record where status-first gives four
    "four_entries_one_record": (
        [("create", [(b"mine", _A), (b"nonul", _B)]),
         ("receive", [_m([b"mine\0not-a-guid", b"nonul", b"new\0" + _DC, b"new\0zz"])], _OK)],
        [(b"new", _C, 0)], {b"mine": _A, b"nonul": _B, b"new": _C}),
    "known_from_create_keys": (
        [("create", [(b"k", _A)]),
         ("receive", [_m([b"k", b"k\0", b"k\0{" + _DB + b"}", b"k\0" + _DB])], _OK)],
        [], {b"k": _A}),
    "known_from_an_earlier_call": (
        [("receive", [_m([b"k\0" + _DA])], _OK),
         ("receive", [_m([b"k", b"k\0zz"]), _m([b"k\0" + _DB[:-1]])], _OK)],
        [(b"k", _A, 0)], {b"k": _A}),
    "known_from_an_earlier_message_of_the_call": (
        [("receive", [_m([b"k\0" + _DA]), _m([b"k", b"k\0zz"])], _OK)],
        [(b"k", _A, 0)], {b"k": _A}),
    "known_from_an_earlier_entry_of_the_message": (
        [("receive", [_m([b"k\0" + _DA.upper(), b"k", b"k\0zz", b"k\0" + _DB])], _OK)],
        [(b"k", _A, 0)], {b"k": _A}),
    # a malformed entry adds nothing, so the key is still unknown when its good entry comes
    "malformed_then_good": (
        [("receive", [_m([b"u\0zz", b"u\0" + _DA])], _OK)],
        [(b"u\0zz", (0, 0), 2), (b"u", _A, 0)], {b"u": _A}),
    "good_then_malformed": (
        [("receive", [_m([b"u\0" + _DA, b"u\0zz"])], _OK)],
        [(b"u", _A, 0)], {b"u": _A}),
    "no_nul_twice_then_good_then_more": (
        [("receive", [_m([b"w", b"w\0yy", b"w\0" + _DB, b"w\0xx"]), _m([b"w\0ww"])], _OK)],
        [(b"w", (0, 0), 1), (b"w\0yy", (0, 0), 2), (b"w", _B, 0)], {b"w": _B}),
    # an entry its own message removes is never seen: it makes nothing known
    "a_removed_good_entry_adds_nothing": (
        [("receive", [_m([b"r\0" + _DA, b"r\0zz"], [b"r\0" + _DA])], _OK)],
        [(b"r\0zz", (0, 0), 2)], {}),
    # the null element is dereferenced (item.Split) before any lookup: status 3 whatever the dictionary holds
    "null_with_the_empty_key_unknown": (
        [("receive", [_m([None, b""])], _OK)],
        [(b"", (0, 0), 3), (b"", (0, 0), 1)], {}),
    "null_with_the_empty_key_known": (
        [("create", [(b"", _A)]),
         ("receive", [_m([None, b"", b"\0zz"])], _OK)],
        [(b"", (0, 0), 3)], {b"": _A}),
    # the all-zero guid is a valid "D" form
    "zero_guid_then_malformed": (
        [("receive", [_m([b"z\0" + b"00000000-0000-0000-0000-000000000000", b"z"])], _OK)],
        [(b"z", _D, 0)], {b"z": _D}),
}


def test_guid_literals():
    assert (R.guid_d(_A), R.guid_d(_B), R.guid_d(_C)) == (_DA, _DB, _DC)


def test_on_next_looks_the_key_up_before_it_parses_the_guid():
    for name, (steps, journal, keys) in ORDER_CASES.items():
        ref = R.KeySpaceRef()
        for st in steps:
            if st[0] == "create":
                ref.create_keys(st[1])
            else:
                assert ref.receive(st[1]) == st[2], name
        assert ref.journal == journal, name
        assert ref.keys == keys, name
