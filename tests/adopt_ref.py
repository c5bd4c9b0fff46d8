"""Python model of CRDT creation on a node (csrc/adopt.hip): the allocation rule, jg_node_register beside it,
jg_node_create_uids and jg_node_adopt_keys, as include/janus_gpu.h states them.  No device, no library.

A node is a dict uid -> (kind, idx) in creation order, the two allocation marks, and its PN-Counter store's shape and
replica table (row -> list of replica Guids in column order).  Uids and replicas are (lo, hi) pairs.
"""
OK, EINVAL, ESTATE = 0, 1, 6  # JG_OK, JG_EINVAL, JG_ESTATE
CREATED, EXISTS = 0, 1  # JG_C_*
ADOPTED, HAVE, NO_TYPE, SKIPPED = 0, 1, 2, 3  # JG_A_*
NO_KIND, NO_IDX = 255, 0xFFFFFFFF
SET_LIMIT = 0x7FFFFFF0


class Refused(Exception):
    def __init__(self, code):
        super().__init__(code)
        self.code = code


class NodeModel:
    def __init__(self, n_keys=0, R=0, has_orset=True):
        self.has = [n_keys > 0, has_orset]  # a store per kind
        self.n_keys, self.R = n_keys, R
        self.uids = {}
        self.next = [0, 0]  # the next PN-Counter row, the next set id
        self.cols = {}
        self.wave_open = False  # a streamed wave of the node, or a wave holding a store

    # jg_node_register: the caller chooses idx
    def register(self, uids, types, idx):
        seen = set()
        for u, t, i in zip(uids, types, idx):
            if u == (0, 0) or t > 1 or not self.has[t] or u in self.uids or u in seen:
                raise Refused(EINVAL)
            if (t == 0 and i >= self.n_keys) or (t == 1 and i >= SET_LIMIT):
                raise Refused(EINVAL)
            seen.add(u)
        for u, t, i in zip(uids, types, idx):
            self.uids[u] = (t, i)
            self.next[t] = max(self.next[t], i + 1)

    # jg_pnc_intern on one row
    def intern(self, row, replica):
        c = self.cols.setdefault(row, [])
        if replica not in c:
            if len(c) >= self.R:
                raise Refused(ESTATE)
            c.append(replica)
        return c.index(replica)

    def _create(self, items, replica, max_keys):
        """items: per entry None (creates nothing) or (uid, kind).  Returns per entry (created, kind, idx) for those that
        name a uid; all or nothing."""
        table, nxt, out, new_rows = dict(self.uids), list(self.next), [], []
        for j, it in enumerate(items):
            if it is None:
                out.append(None)
                continue
            u, k = it
            if u in table:
                out.append((False,) + table[u])
                continue
            if not self.has[k]:
                raise Refused(EINVAL)
            table[u] = (k, nxt[k])
            out.append((True, k, nxt[k]))
            if k == 0:
                new_rows.append((nxt[k], j))
            nxt[k] += 1
        if nxt[1] > SET_LIMIT and nxt[1] > self.next[1]:
            raise Refused(ESTATE)
        n_keys = self.n_keys
        if new_rows and nxt[0] > n_keys:
            if nxt[0] > max_keys:
                raise Refused(ESTATE)
            n_keys = min(max(nxt[0], 2 * n_keys), max_keys)
        if replica is not None:
            for row, j in new_rows:
                c = self.cols.get(row, [])
                if replica[j] not in c and len(c) >= self.R:
                    raise Refused(ESTATE)
        self.uids, self.next, self.n_keys = table, nxt, n_keys
        if replica is not None:
            for row, j in new_rows:
                self.intern(row, replica[j])
        return out

    def create_uids(self, uids, types, replica=None, max_keys=0):
        """-> (status, idx) lists."""
        if self.wave_open and uids:
            raise Refused(EINVAL)
        for u, t in zip(uids, types):
            if u == (0, 0) or t > 1 or not self.has[t]:
                raise Refused(EINVAL)
        out = self._create(list(zip(uids, types)), replica, max_keys)
        return [CREATED if c else EXISTS for c, _, _ in out], [i for _, _, i in out]

    def adopt(self, prospective, records, replica=None, max_keys=0):
        """records: the journal's (key bytes, guid, status) from `from` to `to`.  -> (status, kind, idx) lists."""
        if self.wave_open and records:
            raise Refused(EINVAL)
        items, pre = [], []
        for _, g, st in records:
            if st != 0:
                pre.append(SKIPPED), items.append(None)
            elif g not in prospective.uids:
                pre.append(NO_TYPE), items.append(None)
            else:
                pre.append(None), items.append((g, prospective.uids[g][0]))
        out = self._create(items, replica, max_keys)
        status = [p if o is None else (ADOPTED if o[0] else HAVE) for p, o in zip(pre, out)]
        return status, [NO_KIND if o is None else o[1] for o in out], [NO_IDX if o is None else o[2] for o in out]
