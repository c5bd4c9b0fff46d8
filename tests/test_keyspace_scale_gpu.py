"""GPU: the key space (jg_keyspace_*) past one workgroup, past one scan tile, at capacity and under the 4-bit test
hash, against its restatement (tests/tpset_ref.py KeySpaceRef).  Every comparison is exact and every step is checked
with test_keyspace_gpu.same(): the journal in order, lookup of every known key and of absent probes, the set's sizes,
lookup_all with ordinals and the encoded bytes.

What each test is the first in the suite to run in csrc/keyspace.hip (excl_scan and its kernels: csrc/tpset.hip,
csrc/block_scan.hpp; dict_find, claim_slot and find_slot: csrc/tpset_dict.hpp):
  test_scale_scenario[255 | 256 | 257]   k_ks_parse / _find / _win / _commit / _lookup / _journal with a last workgroup
      that is one lane short, full, and a second workgroup of one lane (the `i >= I.n` guards; blocks_for > 1);
      items_layout's `pow2_at_least(2 * n, 64)` past its 64 slots; a key's entries in different workgroups, so that
      k_ks_find's atomicMin and claim_slot's representative compare decide between lanes that share no workgroup.
  test_scale_scenario[8191 | 8192 | 8193] excl_scan's `n <= 4 * kScanTile` from both sides: at 8193 dict_insert's two
      scans take k_scan_sum / k_scan_apply, and k_ks_commit's bases `n_keys + oa[i]`, `jn + oj[i]` cross scan tiles.
  test_scale_scenario[10241]             a last scan tile that holds one item.
  test_scale_scenario_40000              20 scan tiles, a 131072-slot call-wide table, dict_find over more than 13000
      keys (the second and third receive, create_keys and every lookup), k_ks_local past one workgroup.
  test_journal_paging_at_scale           jg_keyspace_new_keys' excl_scan from `jlen + from` with from odd and large,
      on both scan paths; `nb <= cap_b` refusing a buffer one byte short.
  test_many_messages_in_one_call         on_next with the watermark moving 150 times in one call and keys recurring across
      the messages (every OnNext after the first finds most keys in the dictionary), and jg_keyspace_receive's
      rejection branch with a non-zero *n_new after 150 applied messages.
  test_exactly_full                      dict_insert's `<= cap + 1` with equality on the journal side (8 keys + null).
  test_one_too_many_in_the_middle_message, test_create_keys_past_capacity
      JG_ESTATE through jg_keyspace_receive's `catch (const jg::Error&)` with a code other than JG_EINVAL, and out of
      tpset_apply_ops through jg_keyspace_create_keys' guard; the watermark and n_new after it.
  test_scale_and_random_parity_with_hash_collisions
      dict_find's and SameKey's (k_ks_find through claim_slot, k_ks_win through find_slot) `key == key && klen == klen
      && same_bytes` with the first conjunct true for a sixteenth of all pairs: prefix families (k, k1, k10) make
      klen decide, p...a / p...b the last byte.
Mutants that could index out of bounds are not run on a device; from the code: a wrong scan base in k_scan_apply
shifts every `oa[i]` / `oj[i]` of a later tile, so dictionary ids and journal slots collide and same()'s journal and
lookup compares fail at n >= 8193; dropping `D.klen[d] == klen` makes lookup(b"k") find k1's entry whenever the
4-bit hashes agree, and PROBE's b"k\\0", b"p" * 254 and b"p" * 258 are there for the compares that read one byte
too few or too many."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import janus_gpu as jg
import tpset_ref as R
from test_keyspace_gpu import entry, msg, same

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
M64 = (1 << 64) - 1
ZERO_D = b"00000000-0000-0000-0000-000000000000"
PROBE = (b"absent", b"k\0", b"K", b"k1000000", b"p" * 254, b"p" * 258, b"\xc3", "é2".encode())


def _mix(x):  # splitmix64's finaliser
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ x >> 30) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ x >> 27) * 0x94D049BB133111EB) & M64
    return x ^ x >> 31


def guid(i):
    """Guid number i: distinct for distinct i, never zero."""
    return _mix(2 * i) | 1, _mix(2 * i + 1)


def spelled(key, g, i):
    """A well-formed entry in lower, upper or mixed case, by i."""
    d = R.guid_d(g)
    if i % 3 == 1:
        d = d.upper()
    elif i % 3 == 2:
        d = bytes(c - 32 if k % 2 and 0x61 <= c <= 0x66 else c for k, c in enumerate(d))
    return key + b"\0" + d


N_BAD = 10


def malformed(key, g, v):
    """An entry of `key` that is not key + NUL + "D" form, kind v."""
    d = R.guid_d(g)
    return [key,                                      # no NUL: the key alone (the whole entry is the key)
            key + d,                                  # no NUL: another, longer key
            key + b"\0" + d[:-1],                     # 35 characters
            key + b"\0" + d + b"0",                   # 37
            key + b"\0" + d[:8] + d[9:10] + b"-" + d[10:],  # the first dash one place on
            key + b"\0" + d.replace(b"-", b""),       # "N"
            key + b"\0{" + d + b"}",                  # "B"
            key + b"\0" + d[:5] + b"g" + d[6:],       # not a hex digit
            key + b"\0 " + d + b" ",                  # blanks around it
            key + b"\0",                              # an empty guid segment
            ][v % N_BAD]


def key_pool(k):
    """k distinct keys: the edge keys, then two families in which a key is a prefix of another."""
    long = b"p" * 5000
    edge = [b"", b"k", b"x", long[:255], long[:256], long[:257], long[:4999] + b"a", long[:4999] + b"b",
            "é".encode(), "é1".encode(), "€".encode(), "€é".encode(), "😀".encode(), "😀😀".encode(), b"zero"]
    keys = list(edge)
    i = 0
    while len(keys) < k:
        keys.append(b"k%d" % i if i % 2 else b"a/long/prefix/that/every/key/of/this/family/shares/%d" % (i // 2))
        i += 1
    assert len(set(keys)) == len(keys)
    return keys[:max(k, len(edge))]


def first_message(n, rng):
    """n addSet elements and the removeSet, laid out so that one key's entries meet across workgroups and scan tiles:
    each key three times under three guids, n/3 apart, then permuted, so that the lowest index is not always in the
    first third; every 101st element malformed (of a key that is known by then, or not); every 97th also in removeSet
    and so never seen (the key's first SEEN entry wins, often its second or third); the null element once."""
    keys = key_pool((n - 1) // 3)
    K = len(keys)
    ents = []
    for t in range(3):
        for j, key in enumerate(keys):
            ents.append((key, guid(3 * j + t)))
    ents = [ents[i] for i in rng.permutation(len(ents))]
    add = []
    for i, (key, g) in enumerate(ents):
        if key == b"zero":  # the all-zero guid is a "D" form; its two rivals are not
            z = sum(1 for x in add if x is not None and x.startswith(b"zero\0"))
            add.append([b"zero\0" + ZERO_D, b"zero\0" + ZERO_D[:-1], b"zero\0" + ZERO_D.replace(b"-", b"")][z])
        elif i % 101 == 7:
            add.append(malformed(key, g, i // 101))
        else:
            add.append(spelled(key, g, i))
    add.insert(int(rng.integers(0, len(add))), None)
    j = 0
    while len(add) < n:  # fill to n with malformed entries of keys nobody has
        add.append(malformed(b"filler%d" % j, guid(10 ** 6 + j), j + 2))
        j += 1
    add = add[:n]
    rem = [x for i, x in enumerate(add) if i % 97 == 50 and x is not None and not x.startswith(b"zero\0")]
    return keys, add, rem


def scale_scenario(ctx, n, seed, modes, keep=False):
    """The scenario at n entries per message on one key space per mode; -> (stores, ref) still open when keep."""
    rng = np.random.default_rng(seed)
    keys, add, rem = first_message(n, rng)
    h = n // 2
    third = []
    for i in range(h):
        if i % 2:
            third.append(spelled(keys[int(rng.integers(0, len(keys)))], guid(2 * 10 ** 6 + i), i))
        else:
            third.append(spelled(b"third%d" % (i // 4), guid(2 * 10 ** 6 + i), i))  # each new key twice
    third = [third[i] for i in rng.permutation(h)]
    local = []
    for i in range(h):
        key = [keys[int(rng.integers(0, len(keys)))], b"third%d" % (i // 4), b"local%d" % (i // 6), b"local%d" % (i // 6)][i % 4]
        local.append((key, guid(3 * 10 ** 6 + i)))
    locals_ = sorted({k for k, _ in local if k.startswith(b"local")})[::3][:300]
    later = [spelled(k, guid(4 * 10 ** 6 + i), i) for i, k in enumerate(locals_)] + [spelled(b"fresh", guid(5 * 10 ** 6), 0)]
    m1, m3, m5 = msg(add, rem), msg(third), msg(later)
    every = [x for x in add + third + later if x is not None] + [k + b"\0" + R.guid_d(g) for k, g in local]
    cap_keys, cap_bytes = len(every) + 8, sum(len(x) for x in every) + 64

    ref = R.KeySpaceRef()
    stores = [jg.KeySpace(ctx, cap_keys, cap_bytes) for _ in modes]
    try:
        def receive(m, expect_new=None):
            before = len(ref.journal)
            assert ref.receive([m]) == (None, False)
            n_new = len(ref.journal) - before
            if expect_new is not None:
                assert n_new == expect_new
            for mode, ks in zip(modes, stores):
                assert ks.receive([m], mode=mode) == n_new
                same(ks, ref, PROBE)
            return n_new

        n1 = receive(m1)
        # what the layout is for: first-wins decided across workgroups, removed first entries, both kinds of journal record
        st = [r[2] for r in ref.journal]
        assert st.count(3) == 1 and st.count(1) >= 1 and (st.count(2) >= 1 or n < 300) and n1 == len(st)
        assert ref.keys[b"zero"] == (0, 0) and ref.keys[b""] != (0, 0)
        assert len(ref.keys) >= len(keys) - 3  # all but the few whose three entries were all removed or malformed
        receive(m1, expect_new=0)
        known = set(ref.keys)
        n3 = receive(m3)
        assert n3 == (h + 3) // 4 and all(r[0] not in known and r[0].startswith(b"third") and r[2] == 0 for r in ref.journal[len(ref.journal) - n3:])
        before = len(ref.journal)
        want = ref.create_keys(local)
        assert any(want) and not all(want)
        for ks in stores:
            assert ks.create_keys(local) == want
            same(ks, ref, PROBE)
        assert len(ref.journal) == before
        mine = {k: ref.keys[k] for k, _ in local if k.startswith(b"local")}
        receive(m5, expect_new=1)
        assert ref.journal[-1][0] == b"fresh" and all(ref.keys[k] == g for k, g in mine.items())
        if keep:
            return stores, ref
    except BaseException:
        keep = False
        raise
    finally:
        if not keep:
            for ks in stores:
                ks.close()


# n: the workgroup edge of blocks_for (kBlock = 256), where excl_scan goes from one block to three launches
# (n > 4 * kScanTile = 8192), a last scan tile of one item (5 * 2048 + 1)
@pytest.mark.parametrize("n", [255, 256, 257, 8191, 8192, 8193, 10241])
def test_scale_scenario(ctx, n):
    scale_scenario(ctx, n, 100 + n, (0, 1) if n <= 8193 else (0,))


@pytest.fixture(scope="module")
def big(ctx):
    """n = 40000 (mode 0): about 20 scan tiles, a 131072-slot call-wide table, more than 13000 keys in the dictionary."""
    stores, ref = scale_scenario(ctx, 40000, 40000, (0,), keep=True)
    yield stores[0], ref
    stores[0].close()


def test_scale_scenario_40000(big):
    ks, ref = big
    assert len(ref.keys) > 13000 and len(ref.journal) > 13000
    same(ks, ref, PROBE)


def test_journal_paging_at_scale(big):
    ks, ref = big
    n = len(ref.journal)
    for f in (0, 1, 2047, 2048, 8191, 8192, 8193, n - 8193, n - 1, n):
        assert ks.new_keys(f) == (ref.journal[f:], n)
    with pytest.raises(jg.JanusError) as ei:
        ks.new_keys(n + 1)
    assert ei.value.code == jg.JG_EINVAL
    # the raw ABI with a bytes buffer one byte short
    lib, f = jg.load(), 5
    to, nb = C.c_uint64(), C.c_uint64()
    assert lib.jg_keyspace_new_keys(ks._h, f, C.byref(to), C.byref(nb), None, None, None, None) == jg.JG_OK
    need = sum(len(r[0]) for r in ref.journal[f:])
    assert (to.value, nb.value) == (n, need)
    off, data = np.zeros(n - f + 1, np.uint64), np.zeros(need, np.uint8)
    guids, status = np.zeros(n - f, jg.GUID_DTYPE), np.zeros(n - f, np.uint8)
    nb = C.c_uint64(need - 1)
    assert lib.jg_keyspace_new_keys(ks._h, f, C.byref(to), C.byref(nb), jg._ptr(off), jg._ptr(data), jg._ptr(guids), jg._ptr(status)) == jg.JG_ESTATE
    assert ks.new_keys(0) == (ref.journal, n)
    nb = C.c_uint64(need)
    assert lib.jg_keyspace_new_keys(ks._h, f, C.byref(to), C.byref(nb), jg._ptr(off), jg._ptr(data), jg._ptr(guids), jg._ptr(status)) == jg.JG_OK
    assert nb.value == need and data.tobytes() == b"".join(r[0] for r in ref.journal[f:]) and [int(x) for x in status] == [r[2] for r in ref.journal[f:]]
    same(ks, ref, PROBE)


def test_many_messages_in_one_call(ctx):
    """200 messages of about 5 entries over 120 recurring keys in one call.  Message m removes what message m - 2 added
    first (seen all the same) and, when m % 7 == 3, what message m + 1 adds first (never seen); message 150 is malformed."""
    rng = np.random.default_rng(200)
    keys = key_pool(120)
    adds = [[spelled(keys[int(k)], guid(1000 * m + e), m + e) for e, k in enumerate(rng.integers(0, len(keys), int(rng.integers(3, 8))))] for m in range(200)]
    for m in range(0, 200, 23):
        adds[m].append(malformed(keys[m % len(keys)], guid(m), m))
    adds[77].append(None)
    msgs = []
    for m in range(200):
        rem = [adds[m - 2][0]] if m >= 2 else []
        if m % 7 == 3 and m + 1 < 200:
            rem.append(adds[m + 1][0])
        msgs.append(msg(adds[m], rem))
    msgs[150] = msgs[150][:-2]  # the removeSet's ']' and the '}' are gone
    for mode in (0, 1):
        ref = R.KeySpaceRef()
        with jg.KeySpace(ctx, 2048, 1 << 20) as ks:
            assert ref.receive(msgs) == (150, False)
            n_new = len(ref.journal)
            assert n_new > 100 and any(r[2] for r in ref.journal)
            never = [adds[m + 1][0] for m in range(3, 149, 7)]
            assert all(x in ref.set.rem_set for x in never)
            with pytest.raises(jg.JanusError) as ei:
                ks.receive(msgs, mode=mode)
            assert (ei.value.code, ei.value.bad_msg, ei.value.partial, ei.value.n_new) == (jg.JG_EINVAL, 150, False, n_new)
            same(ks, ref, PROBE)
            assert ref.receive(msgs[151:]) == (None, False)
            assert ks.receive(msgs[151:], mode=mode) == len(ref.journal) - n_new
            same(ks, ref, PROBE)


# ---- capacity: KeySpace(ctx, 8, ...) -----------------------------------------------------------------------------
E8 = [entry(b"key%d" % i, guid(i)) for i in range(8)]
BYTES8 = sum(len(x) for x in E8)


def estate(call):
    with pytest.raises(jg.JanusError) as ei:
        call()
    assert ei.value.code == jg.JG_ESTATE
    return ei.value


def test_exactly_full(ctx):
    """Eight keys and the null element in a key space of eight: the dictionary holds 8 and the journal 9."""
    for mode in (0, 1):
        ref = R.KeySpaceRef()
        with jg.KeySpace(ctx, 8, BYTES8) as ks:
            m = msg(E8[:5] + [None] + E8[5:])
            assert ref.receive([m]) == (None, False)
            assert len(ref.keys) == 8 and len(ref.journal) == 9
            assert ks.receive([m], mode=mode) == 9
            same(ks, ref, PROBE)
            assert ks.set.size() == (9, 0, BYTES8)


@pytest.mark.parametrize("what", ["string", "byte"])
def test_one_too_many_in_the_middle_message(ctx, what):
    """Three messages, the second of which does not fit (by one string, by one byte): JG_ESTATE, n_new counts the first
    message's records and the state is the reference's after the first message alone; then a message that fits."""
    first, fits = [msg(E8[:3] + [b"nonul"])], [msg(E8[3:7])]
    if what == "string":
        cap_bytes, middle = 1 << 12, msg(E8[3:])  # 4 + 5 strings
    else:
        cap_bytes = BYTES8 + len(b"nonul")
        middle = msg(E8[3:7] + [E8[7] + b"\0"])  # 8 strings, one byte past cap_bytes
    for mode in (0, 1):
        ref = R.KeySpaceRef()
        with jg.KeySpace(ctx, 9 if what == "byte" else 8, cap_bytes) as ks:
            assert ref.receive(first) == (None, False)
            e = estate(lambda: ks.receive(first + [middle, msg([entry(b"after", guid(20))])], mode=mode))
            assert e.n_new == len(ref.journal) == 4
            same(ks, ref, PROBE + (b"key3", b"key7", b"after"))
            assert ref.receive(fits) == (None, False)
            assert ks.receive(fits, mode=mode) == 4
            same(ks, ref, PROBE)


def test_create_keys_past_capacity(ctx):
    ref = R.KeySpaceRef()
    with jg.KeySpace(ctx, 8, 1 << 12) as ks:
        pairs = [(b"key%d" % i, guid(i)) for i in range(6)]
        assert ks.create_keys(pairs) == ref.create_keys(pairs)
        same(ks, ref, PROBE)
        over = [(b"over%d" % i, guid(30 + i)) for i in range(3)]
        estate(lambda: ks.create_keys(over))
        assert ks.lookup([k for k, _ in over]) == [None] * 3
        same(ks, ref, PROBE)
        ok = over[:2]
        assert ks.create_keys(ok) == ref.create_keys(ok) == [True, True]
        same(ks, ref, PROBE)


# ---- under the 4-bit hash ------------------------------------------------------------------------------------------
def test_scale_and_random_parity_with_hash_collisions():
    """scale_scenario at 1800 entries and test_keyspace_gpu's random-parity body against the test build, whose string
    hash keeps 4 bits (-DJANUS_TEST_HOOKS; key_hash goes through it): the dictionary, the call-wide table and the set's
    own table are 16 long probe chains, and the length and byte compares decide every lookup.  In a child process
    through JANUS_GPU_LIB, as test_tpset_gpu.test_random_parity_with_hash_collisions."""
    lib = ROOT / "janus-crdt_amd" / "lib" / "libjanusgpu_test.so"
    assert lib.exists(), "the test build is made by __graft_entry__.build()"
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import janus_gpu as jg, test_keyspace_gpu as t, test_keyspace_scale_gpu as s\n"
            "assert 'libjanusgpu_test' in str(jg.LIB_PATH)\n"
            "ctx = jg.Context(0)\ns.scale_scenario(ctx, 1800, 18, (0, 1))\nt.journal_paging_and_random_parity(ctx)\nctx.close()\nprint('PARITY OK')\n"
            % (str(ROOT / "janus-crdt_amd"), str(ROOT / "tests")))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240, env=dict(os.environ, JANUS_GPU_LIB=str(lib)),
                         cwd=str(ROOT / "tests"))
    assert out.returncode == 0 and "PARITY OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
