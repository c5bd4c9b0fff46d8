"""Python restatements of csrc/table_hash.hpp — seq_hash (the safe-update tracker's slots) and uid_hash (the node's uid
table and the shard rule) — and their inverses.  Both are bijections on 64 bits (uid_hash for a fixed hi, and for
lo == 0 as a function of hi), so a test chooses the slot a key homes to: a target hash whose low 20 bits are all ones
lands in the LAST slot of every table of up to 2^20 slots, whatever capacity the library picked, and every probe from
there wraps to slot 0.  tests/test_table_hash.py holds the restatements to the C++ (build/test_table_hash).
"""
M64 = (1 << 64) - 1

SEQ_C1, SEQ_C2 = 0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53
UID_G, UID_M = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9
SEQ_C1_INV, SEQ_C2_INV, UID_G_INV, UID_M_INV = (pow(c, -1, 1 << 64) for c in (SEQ_C1, SEQ_C2, UID_G, UID_M))

LAST = 0xFFFFF  # the low 20 bits of a hash that homes to the last slot


def seq_hash(x):
    x ^= x >> 33
    x = x * SEQ_C1 & M64
    x ^= x >> 33
    x = x * SEQ_C2 & M64
    return x ^ (x >> 33)


def uid_hash(lo, hi):
    x = lo ^ (hi * UID_G & M64)
    x ^= x >> 31
    x = x * UID_M & M64
    x ^= x >> 29
    return x


def shard_of_uid(lo, hi, world):
    return 0 if world <= 1 else (uid_hash(lo, hi) >> 7) % world


def _unxorshift(y, s):
    """x with x ^ (x >> s) == y."""
    x, t = y, y >> s
    while t:
        x ^= t
        t >>= s
    return x


def seq_unhash(h):
    x = _unxorshift(h, 33)
    x = x * SEQ_C2_INV & M64
    x = _unxorshift(x, 33)
    x = x * SEQ_C1_INV & M64
    return _unxorshift(x, 33)


def _uid_mix_inv(h):
    x = _unxorshift(h, 29)
    x = x * UID_M_INV & M64
    return _unxorshift(x, 31)


def uid_unhash(h, hi):
    """lo with uid_hash(lo, hi) == h."""
    return _uid_mix_inv(h) ^ (hi * UID_G & M64)


def uid_unhash_lo0(h):
    """hi with uid_hash(0, hi) == h."""
    return _uid_mix_inv(h) * UID_G_INV & M64


def last_slot_target(j):
    """The j-th hash value that homes to the last slot of any table of up to 2^20 slots."""
    return (j << 20) | LAST


def clustered_seqs(j0, n):
    """n tracker identities homing to the last slot (targets j0 .. j0 + n - 1); never a reserved identity."""
    out = [seq_unhash(last_slot_target(j)) for j in range(j0, j0 + n)]
    assert all(s not in (0, M64) for s in out) and len(set(out)) == n
    return out


def clustered_uids(j0, his):
    """One (lo, hi) per given hi, homing to the last slot (targets j0 ..).  hi == 0 is allowed (lo is then the whole
    key); a None asks for the uid with lo == 0."""
    out = []
    for k, hi in enumerate(his):
        h = last_slot_target(j0 + k)
        u = (0, uid_unhash_lo0(h)) if hi is None else (uid_unhash(h, hi), hi)
        assert u != (0, 0) and uid_hash(*u) == h
        out.append(u)
    assert len(set(out)) == len(out)
    return out
