"""The OR-Set record walk in its prefix-sum form, in Python, beside a sequential transcription of the
host walk it replaces.  Both take a stored state (add and tombstone records) and a batch of ops (1 Add, 2 Remove,
3 Clear, 4 the internal read) and return what jg_orset_apply_ops_ords computes before the union: the results, the
batch's add and tombstone records with their batch ords, the limits after each op, and the Cleared sets.

walk_prefix() follows the device walk step by step: every per-op quantity is a count over the ops before it in
(set, elem, epoch, op index) order, never a state carried from op to op."""
from itertools import accumulate

import numpy as np

NULL_ELEM = 0xFFFFFFFF
REC_DTYPE = np.dtype([("key", "<u8"), ("tag_lo", "<u8"), ("tag_hi", "<u8"), ("ord", "<u8")])


def _runs(recs):
    """key -> [(ord, lo, hi)] of a stored stream."""
    out = {}
    for r in recs:
        out.setdefault(int(r["key"]), []).append((int(r["ord"]), int(r["tag_lo"]), int(r["tag_hi"])))
    return out


def _excl(flags):
    return [0] + list(accumulate(flags))[:-1] if flags else []


def walk_prefix(A, R, sets, elems, ops, lo, hi):
    n = len(ops)
    sets, elems, ops = [int(x) for x in sets], [int(x) for x in elems], [int(x) for x in ops]
    tag = [(int(a), int(b)) for a, b in zip(lo, hi)]
    key = [(sets[i] << 32) | elems[i] for i in range(n)]
    runs_a, runs_r = _runs(A), _runs(R)

    # order 1: (set, op index); the Clear epoch of an op = the Clears of its set before it
    p1 = sorted(range(n), key=lambda i: (sets[i], i))
    epoch, n_clears = [0] * n, {}
    for i in p1:
        epoch[i] = n_clears.get(sets[i], 0)
        if ops[i] == 3:
            n_clears[sets[i]] = epoch[i] + 1
    keep = [epoch[i] == n_clears.get(sets[i], 0) for i in range(n)]  # no Clear of the set follows
    cleared = sorted(n_clears)

    # order 2: (set, elem, epoch, op index) = (key, op index), epochs being monotone in the op index
    p2 = sorted(range(n), key=lambda i: (key[i], i))
    seg = [0] * n  # first position of the position's (key, epoch) segment
    for p in range(n):
        same = p > 0 and key[p2[p]] == key[p2[p - 1]] and epoch[p2[p]] == epoch[p2[p - 1]]
        seg[p] = seg[p - 1] if same else p
    removed = {key[i] for i in range(n) if ops[i] == 2}
    named = removed | {key[i] for i in range(n) if ops[i] == 4}

    # first occurrence of a tag within a (key, epoch)
    first, seen = [False] * n, set()
    for i in range(n):
        if ops[i] == 1:
            k = (key[i], epoch[i], tag[i])
            first[i] = k not in seen
            seen.add(k)

    # the stored state a segment starts from: only epoch 0 of a key a Remove or a read names
    def base(i):
        if epoch[i] != 0 or key[i] not in named:
            return set(), set(), []
        a, r = runs_a.get(key[i], []), runs_r.get(key[i], [])
        rt = {(x[1], x[2]) for x in r}
        u0 = [(x[1], x[2]) for x in sorted(a) if (x[1], x[2]) not in rt]
        return {(x[1], x[2]) for x in a}, rt, u0

    issue_s, fill, uadd, issue_w = [0] * n, [0] * n, [0] * n, [0] * n  # by position of order 2 (issue_w: by op)
    for p in range(n):
        i = p2[p]
        if ops[i] == 1:
            a0, r0, _ = base(i)
            issue_s[p] = int(first[i] and tag[i] not in a0)
            fill[p] = int(issue_s[p] and tag[i] in r0)
            uadd[p] = issue_s[p] - fill[p]
            issue_w[i] = issue_s[p] if key[i] in removed else int(first[i])
    isx, flx, uax = _excl(issue_s), _excl(fill), _excl(uadd)

    def prev_remove(p):
        for q in range(p - 1, seg[p] - 1, -1):
            if ops[p2[q]] == 2:
                return q
        return None

    def next_remove(p):
        for q in range(p, n):
            if seg[q] != seg[p]:
                return None
            if ops[p2[q]] == 2:
                return q
        return None

    def state(p):
        i, s = p2[p], seg[p]
        a0, r0, u0 = base(i)
        q = prev_remove(p)
        nA = len(a0) + isx[p] - isx[s]
        m = len(r0 - a0) - (flx[p] - flx[s])
        if q is None:
            return nA, len(r0), m, len(u0) + uax[p] - uax[s]
        return nA, len(r0) + len(u0) + uax[q] - uax[s], m, uax[p] - uax[q]

    res, cnt_r = [1] * n, [0] * n
    for p in range(n):
        i = p2[p]
        if ops[i] in (2, 4):
            nA, nR, m, u = state(p)
            res[i] = int((m > 0 or u > 0) if elems[i] == NULL_ELEM else (nA > 0 and (nR == 0 or m > 0 or u > 0)))
            if ops[i] == 2:
                cnt_r[i] = u

    # ords: a second prefix sum, over the records each op issues, in (set, op index) order
    ax = _excl([issue_w[i] for i in p1])
    rx = _excl([cnt_r[i] for i in p1])
    abase, rbase, add_lim, rem_lim = [0] * n, [0] * n, [0] * n, [0] * n
    for x, i in enumerate(p1):
        abase[i], rbase[i] = ax[x], rx[x]
        add_lim[i], rem_lim[i] = ax[x] + issue_w[i], rx[x] + cnt_r[i]

    adds = [(key[i], tag[i][0], tag[i][1], abase[i]) for i in range(n) if issue_w[i] and keep[i]]
    tombs = []
    for p in range(n):
        i = p2[p]
        if uadd[p]:
            r = next_remove(p)
            if r is not None and keep[p2[r]]:
                q, s = prev_remove(p), seg[p]
                at = uax[p] - uax[q] if q is not None else len(base(i)[2]) + uax[p] - uax[s]
                tombs.append((key[i], tag[i][0], tag[i][1], rbase[p2[r]] + at))
        if ops[i] == 2 and prev_remove(p) is None and keep[i]:
            for at, t in enumerate(base(i)[2]):
                tombs.append((key[i], t[0], t[1], rbase[i] + at))
    return (np.array(res, np.uint8), np.array(sorted(adds), REC_DTYPE), np.array(sorted(tombs), REC_DTYPE),
            np.array(add_lim, np.uint64), np.array(rem_lim, np.uint64), cleared)


def walk_sequential(A, R, sets, elems, ops, lo, hi):
    """The host walk (csrc/orset.hip apply_ops), op by op over explicit tag sets."""
    n = len(ops)
    sets, elems, ops = [int(x) for x in sets], [int(x) for x in elems], [int(x) for x in ops]
    runs_a, runs_r = _runs(A), _runs(R)
    key = [(sets[i] << 32) | elems[i] for i in range(n)]
    removed = {key[i] for i in range(n) if ops[i] == 2}
    named = removed | {key[i] for i in range(n) if ops[i] == 4}
    res, add_lim, rem_lim = [1] * n, [0] * n, [0] * n
    adds, tombs, cleared = [], [], []
    next_a = next_r = 0

    def load(k):
        a = [(x[1], x[2]) for x in sorted(runs_a.get(k, []))]
        r = [(x[1], x[2]) for x in sorted(runs_r.get(k, []))]
        return {"add": a, "rem": r, "ah": set(a), "rh": set(r)}

    def empty():
        return {"add": [], "rem": [], "ah": set(), "rh": set()}

    def present(e, st):
        return st["ah"] != st["rh"] if e == NULL_ELEM else bool(st["ah"]) and (not st["rh"] or st["ah"] != st["rh"])

    for sid in sorted(set(sets)):
        st, rd, was_cleared, mine_a, mine_r = {}, {}, False, [], []
        for i in [j for j in range(n) if sets[j] == sid]:
            k, t = key[i], (int(lo[i]), int(hi[i]))
            if ops[i] != 3 and k not in st:
                st[k] = load(k) if (not was_cleared and k in removed) else empty()
            if ops[i] in (1, 4) and k in named and k not in removed and k not in rd:
                rd[k] = empty() if was_cleared else load(k)
            if ops[i] == 1:
                if t not in st[k]["ah"]:
                    st[k]["ah"].add(t)
                    st[k]["add"].append(t)
                    mine_a.append((k, t[0], t[1], next_a))
                    next_a += 1
                if k in rd:
                    rd[k]["ah"].add(t)
            elif ops[i] == 2:
                res[i] = int(present(elems[i], st[k]))
                if res[i]:
                    for u in st[k]["add"]:
                        if u not in st[k]["rh"]:
                            st[k]["rh"].add(u)
                            st[k]["rem"].append(u)
                            mine_r.append((k, u[0], u[1], next_r))
                            next_r += 1
            elif ops[i] == 4:
                res[i] = int(present(elems[i], st[k] if k in removed else rd[k]))
            else:
                st, rd, mine_a, mine_r, was_cleared = {}, {}, [], [], True
            add_lim[i], rem_lim[i] = next_a, next_r
        adds += mine_a
        tombs += mine_r
        if was_cleared:
            cleared.append(sid)
    return (np.array(res, np.uint8), np.array(sorted(adds), REC_DTYPE), np.array(sorted(tombs), REC_DTYPE),
            np.array(add_lim, np.uint64), np.array(rem_lim, np.uint64), cleared)


def union(A, R, adds, tombs, cleared):
    """(the store minus the Cleared sets) ∪ the batch's records, which take ords after the store's."""
    out = []
    for old, new in ((A, adds), (R, tombs)):
        old = np.ascontiguousarray(old, REC_DTYPE)
        nxt = int(old["ord"].max()) + 1 if old.size else 0
        have = {(int(r["key"]), int(r["tag_lo"]), int(r["tag_hi"])) for r in old}
        rows = [tuple(int(v) for v in r) for r in old if (int(r["key"]) >> 32) not in cleared]
        rows += [(int(r["key"]), int(r["tag_lo"]), int(r["tag_hi"]), int(r["ord"]) + nxt) for r in new
                 if (int(r["key"]), int(r["tag_lo"]), int(r["tag_hi"])) not in have or (int(r["key"]) >> 32) in cleared]
        out.append(np.array(sorted(rows), REC_DTYPE))
    return out[0], out[1]
