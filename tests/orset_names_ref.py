"""Test-only restatement of ORSet<string> over strings and of the element-id rule of the by-name entry points.

ORSetStr  a literal transcription of MergeSharp/MergeSharp/CRDTs/ORSet.cs:134-237 (Add, Remove, Clear, LookupAll,
          Contains) over insertion-ordered dicts: a C# Dictionary that only ever loses keys through Clear() enumerates
          in insertion order, and so does a HashSet that is never removed from.  Elements are bytes, None is the C# null
          element; tags (Guid.NewGuid() in the reference) are passed in.
Interner  the id rule of jg_orset_apply_ops_names, which is that of the host mirror (elem_id_in / prepare,
          janus-crdt_amd/host/janus_host.cpp): per set, an Add takes the name's live id or the set's next id (ids only
          grow, also across Clear); a Remove takes the live id or NEVER; a Clear drops the set's live names.
"""

NULL_ELEM = 0xFFFFFFFF
NEVER = NULL_ELEM - 1  # "never allocated": the id no record carries
ADD, REMOVE, CLEAR = 1, 2, 3


class ORSetStr:
    def __init__(self):
        self.addSet, self.removeSet = {}, {}          # item -> {tag: None}
        self.nullAddGuid, self.nullRemoveGuid = {}, {}

    def Add(self, item, tag):                          # ORSet.cs:134-153
        if item is None:
            self.nullAddGuid.setdefault(tag)
            return True
        if item in self.addSet:
            self.addSet[item].setdefault(tag)
        else:
            self.addSet[item] = {tag: None}
        return True

    def Remove(self, item):                            # :161-186
        if item is None and item in self.LookupAll():
            for t in self.nullAddGuid:
                self.nullRemoveGuid.setdefault(t)
            return True
        if not self.Contains(item):
            return False
        to_remove = self.addSet[item]
        if item in self.removeSet:
            for t in to_remove:
                self.removeSet[item].setdefault(t)
        else:
            self.removeSet[item] = dict.fromkeys(to_remove)
        return True

    def Clear(self):                                   # :192-198
        self.addSet.clear()
        self.removeSet.clear()
        self.nullAddGuid.clear()
        self.nullRemoveGuid.clear()

    def LookupAll(self):                               # :204-227
        in_only_add = [k for k in self.addSet if k not in self.removeSet]
        in_both = [k for k, v in self.addSet.items() if k in self.removeSet and set(v) != set(self.removeSet[k])]
        null_val = [None] if set(self.nullRemoveGuid) != set(self.nullAddGuid) else []
        return list(dict.fromkeys(in_only_add + in_both + null_val))  # Union: distinct, first occurrence kept

    def Contains(self, item):                          # :234-237
        return item in self.LookupAll()

    @property
    def Count(self):
        return len(self.LookupAll())

    def apply(self, op, item, tag):
        if op == ADD:
            return self.Add(item, tag)
        if op == REMOVE:
            return self.Remove(item)
        self.Clear()
        return True


class Interner:
    def __init__(self):
        self.live = {}     # set -> {name: id}
        self.next_id = {}  # set -> next id (only grows)
        self.log = []      # (set, id, name): every name ever issued, in issue order

    def id_of(self, s, name):
        """The live id of a name (NULL_ELEM for None, NEVER if the set lacks it): jg_orset_resolve_names."""
        return NULL_ELEM if name is None else self.live.get(s, {}).get(name, NEVER)

    def adopt(self, s, i, name):
        """A name another writer issued (a wave commit, jg_orset_names_sync)."""
        self.live.setdefault(s, {})[name] = i
        self.next_id[s] = max(self.next_id.get(s, 0), i + 1)
        self.log.append((s, i, name))

    def clear(self, s):
        self.live[s] = {}

    def op(self, s, op, name):
        """The id an op addresses, and the event it causes for a caller that mirrors the table through
        jg_orset_names_sync: ("name", set, id, bytes) / ("clear", set) / None."""
        if op == CLEAR:
            self.clear(s)
            return 0, ("clear", s)
        if name is None:
            return NULL_ELEM, None
        live = self.live.setdefault(s, {})
        if name in live:
            return live[name], None
        if op == REMOVE:
            return NEVER, None
        i = self.next_id.get(s, 0)
        live[name] = i
        self.next_id[s] = i + 1
        self.log.append((s, i, name))
        return i, ("name", s, i, name)
