"""GPU: KeySpaceManager's state on the device (jg_keyspace_*) against its restatement (tests/tpset_ref.py KeySpaceRef),
whose OnNext runs message by message, in the reference's order (ContainsKey before Guid.Parse), with the documented
departure for malformed entries of unknown keys."""
import numpy as np
import pytest

import janus_gpu as jg
import tpset_ref as R
from test_tpset import ORDER_CASES

pytestmark = pytest.mark.gpu

G = [(0x1111111111111111 * k & 0xFFFFFFFFFFFFFFFF, 0x0123456789ABCDEF ^ k * 0x9E3779B97F4A7C15 & 0xFFFFFFFFFFFFFFFF) for k in range(1, 40)]


def entry(key, g, upper=False):
    d = R.guid_d(g)
    return key + b"\0" + (d.upper() if upper else d)


def msg(add, rem=()):
    return R.encode_msg(list(add), list(rem))


def same(ks, ref, probe=()):
    journal, to = ks.new_keys(0)
    assert journal == ref.journal and to == len(ref.journal)
    keys = list(ref.keys) + list(probe)
    assert ks.lookup(keys) == [ref.keys.get(k) for k in keys]
    assert ks.set.size() == ref.set.size()
    assert ks.set.lookup_all(with_ords=True) == ref.set.lookup_all(with_ords=True)
    assert ks.set.encode_json() == ref.set.encode()


def both(ctx, steps, probe=(b"nokey", b"")):
    """steps: ("create", pairs) | ("receive", msgs, expected (bad, partial)); checked after every step, both modes."""
    for mode in (0, 1):
        ref = R.KeySpaceRef()
        with jg.KeySpace(ctx, 256, 1 << 16) as ks:
            for st in steps:
                if st[0] == "create":
                    assert ks.create_keys(st[1]) == ref.create_keys(st[1])
                else:
                    before = len(ref.journal)
                    exp = ref.receive(st[1])
                    assert exp == st[2]
                    if exp[0] is None:
                        assert ks.receive(st[1], mode=mode) == len(ref.journal) - before
                    else:
                        with pytest.raises(jg.JanusError) as ei:
                            ks.receive(st[1], mode=mode)
                        assert (ei.value.code, ei.value.bad_msg, ei.value.partial, ei.value.n_new) == (jg.JG_EINVAL, exp[0], exp[1], len(ref.journal) - before)
                same(ks, ref, probe)
    return ref


def test_first_guid_wins_inside_and_across_messages(ctx):
    ref = both(ctx, [("receive", [msg([entry(b"k", G[0]), entry(b"k", G[1]), entry(b"j", G[2], upper=True)]), msg([entry(b"k", G[3]), entry(b"i", G[4])])],
                      (None, False)),
                     ("receive", [msg([entry(b"j", G[5])])], (None, False))])
    assert ref.keys == {b"k": G[0], b"j": G[2], b"i": G[4]}
    assert [r[0] for r in ref.journal] == [b"k", b"j", b"i"]


def test_removed_entries(ctx):
    """An entry in both arrays of one message is never seen, not by a later message either; one removed by a later
    message of the same call is seen."""
    a, b, c = entry(b"a", G[0]), entry(b"b", G[1]), entry(b"c", G[2])
    ref = both(ctx, [("receive", [msg([a, b], [a]), msg([c], [b]), msg([a, entry(b"a", G[3])])], (None, False))])
    assert ref.keys == {b"b": G[1], b"c": G[2], b"a": G[3]}


def test_local_create_then_the_same_key_from_a_peer(ctx):
    ref = both(ctx, [("create", [(b"mine", G[0]), (b"mine", G[1]), (b"other", G[2])]),
                     ("receive", [msg([entry(b"mine", G[3]), entry(b"theirs", G[4]), entry(b"other", G[2])])], (None, False)),
                     ("create", [(b"theirs", G[5]), (b"new", G[6])])])
    assert ref.keys == {b"mine": G[0], b"other": G[2], b"theirs": G[4], b"new": G[6]}
    assert [r[0] for r in ref.journal] == [b"theirs"]  # local keys are in the dictionary already: nothing to journal


def test_malformed_entries_are_journalled_and_skipped(ctx):
    bad_guid = b"g\0" + R.guid_d(G[0])[:-1] + b"x"
    braces = b"h\0{" + R.guid_d(G[1]) + b"}"
    three = b"t\0" + R.guid_d(G[2]) + b"\0tail"
    ref = both(ctx, [("receive", [msg([b"nonul", bad_guid, None, braces, three, b"", entry(b"ok", G[3])])], (None, False))])
    assert [r[2] for r in ref.journal] == [1, 2, 3, 2, 0, 1, 0]
    assert ref.keys == {b"t": G[2], b"ok": G[3]}


def test_rejected_and_partial_messages(ctx):
    """A rejected message stops the call before its OnNext; what a partial merge added is seen by the next call."""
    a, b, c = entry(b"a", G[0]), entry(b"b", G[1]), entry(b"c", G[2])
    ref = both(ctx, [("receive", [msg([a]), b'{"addSet":["' + R.escape(b) + b'"]}', msg([c])], (1, True)),
                     ("receive", [msg([c]), b'{"addSet":[1],"removeSet":[]}'], (1, False))])
    assert ref.keys == {b"a": G[0], b"b": G[1], b"c": G[2]}
    assert [r[0] for r in ref.journal] == [b"a", b"b", b"c"]


def journal_paging_and_random_parity(ctx):
    rng = np.random.default_rng(9)
    keys = [b"key%03d" % i for i in range(60)] + [b"", "ключ€".encode()]
    ref = R.KeySpaceRef()
    with jg.KeySpace(ctx, 1024, 1 << 17) as ks:
        marks = [0]
        for step in range(12):
            pick = lambda k: [(keys[i], G[int(rng.integers(0, len(G)))]) for i in rng.integers(0, len(keys), k)]
            if step % 3 == 0:
                p = pick(int(rng.integers(1, 12)))
                assert ks.create_keys(p) == ref.create_keys(p)
            else:
                msgs = []
                for _ in range(int(rng.integers(1, 4))):
                    add = [entry(k, g, upper=bool(rng.integers(0, 2))) for k, g in pick(int(rng.integers(0, 15)))]
                    old = [x for x in ref.set.add_set if x is not None]
                    rem = [old[i] for i in rng.integers(0, len(old), 2)] if old and rng.integers(0, 2) else []
                    msgs.append(msg(add + ([b"junk%d" % step] if step == 4 else []), rem + add[:1]))
                before = len(ref.journal)
                assert ref.receive(msgs) == (None, False)
                assert ks.receive(msgs, mode=step % 2) == len(ref.journal) - before
            marks.append(len(ref.journal))
            same(ks, ref, [b"absent"])
        assert len(ref.journal) > 20
        for f in sorted(set(marks)):
            page, to = ks.new_keys(f)
            assert (page, to) == (ref.journal[f:], len(ref.journal))
        with pytest.raises(jg.JanusError):
            ks.new_keys(len(ref.journal) + 1)


def test_journal_paging_and_random_parity(ctx):
    journal_paging_and_random_parity(ctx)


@pytest.mark.parametrize("name", list(ORDER_CASES))
def test_known_key_is_skipped_before_its_guid_is_parsed(ctx, name):
    """KeySpaceManager.cs:163-166: ContainsKey comes before Split(...)[1] and Guid.Parse.  The cases and their
    journals, worked out by hand, are test_tpset.ORDER_CASES; the known key comes from create_keys, from an earlier
    call, from an earlier message of the call and from an earlier entry of the message."""
    steps, journal, keys = ORDER_CASES[name]
    ref = both(ctx, steps, probe=(b"nokey", b"", b"k", b"u", b"w", b"r", b"new"))
    assert ref.journal == journal and ref.keys == keys


def test_kat_keyspace_binary():
    """host/kat_keyspace: the reference's 2PSetTests scenarios on the device and four-node key discovery through
    janus::GpuKeySpace; every scenario prints PASS."""
    import subprocess
    from pathlib import Path
    exe = Path(__file__).resolve().parents[1] / "janus-crdt_amd" / "build" / "kat_keyspace"
    assert exe.exists(), "built by __graft_entry__.build()"
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith(("PASS", "FAIL"))]
    assert out.returncode == 0 and len(lines) == 5 and all(ln.startswith("PASS") for ln in lines), out.stdout[-2000:] + out.stderr[-2000:]
