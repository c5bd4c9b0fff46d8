"""Test-only sequential model of jg_node_exec_keys: the commands of a batch one at a time, in batch
order, as the reference's server runs them (PNCounterCommand.cs:27-53, ORSetCommand.cs:28-69, under lock (instance)).

A write is SafeCRDT.Update: PNCounterWrapper.Update / ORSetWrapper.Update's verdict (`write_rule`), then
oracle_ref.pnc_apply_ops on the row at the store's width, or orset_names_ref.ORSetStr with the Interner's id rule.
A read is SafeCRDT.QueryProspective: oracle_ref.pnc_values of the row as it stands at that point (Get's checked sums),
or ORSetStr.Contains of the element at that point.  Nothing here knows about prefixes, rounds or lists.
"""
import numpy as np

import oracle_ref as orc
from orset_names_ref import ADD, CLEAR, NEVER, NULL_ELEM, REMOVE, Interner, ORSetStr

Q_OK, Q_NO_KEY, Q_NO_CRDT, Q_OVERFLOW, Q_NO_ARG = range(5)
U_OK, U_NO_KEY, U_NO_CRDT, U_BAD_ARG, U_BAD_OP = range(5)
NO_IDX = 0xFFFFFFFF
INC, DEC = 1, 2
GUID_DTYPE = np.dtype([("lo", "<u8"), ("hi", "<u8")])


class _Null:
    def __repr__(self):
        return "NULL"


def _b(x):
    return x.encode() if isinstance(x, str) else bytes(x)


def _is_int(a):
    return isinstance(a, (int, np.integer)) and not isinstance(a, bool)


def write_rule(t, op, arg, null):
    """PNCounterWrapper.Update (PNCounterWrapper.cs:33-48) evaluates (int)args[0] before its switch; ORSetWrapper.Update
    (ORSetWrapper.cs:30-47) switches first, and Clear reads no argument."""
    if t == 0:
        if not _is_int(arg):
            return U_BAD_ARG
        return U_OK if op in (INC, DEC) else U_BAD_OP
    if op not in (ADD, REMOVE, CLEAR):
        return U_BAD_OP
    if op == CLEAR or arg is null or isinstance(arg, (str, bytes)):
        return U_OK
    return U_BAD_ARG


class ExecModel:
    """guid: key bytes -> (lo, hi); reg: (lo, hi) -> (type, idx), both shared with the caller and read at every run.
    P, N: the PN-Counter rows (copied; None without a store).  null: the object that stands for the C# null argument."""

    def __init__(self, guid, reg, P=None, N=None, null=None, orset=True):
        self.guid, self.reg = guid, reg
        self.P, self.N = (None, None) if P is None else (P.copy(), N.copy())
        self.null = _Null() if null is None else null
        self.orset = orset
        self.sets, self.it = {}, Interner()

    def run(self, cmds, lo, hi, col=0):
        """cmds: [(key, read, op, arg)]; lo / hi: one tag per command.  Returns exec_keys' per-command outputs."""
        n = len(cmds)
        out = {"status": np.zeros(n, np.uint8), "result": np.zeros(n, np.uint8), "value": np.zeros(n, np.int64),
               "kind": np.full(n, 255, np.uint8), "idx": np.full(n, NO_IDX, np.uint32), "elem": np.full(n, NEVER, np.uint32),
               "guid": np.zeros(n, GUID_DTYPE)}
        for i, (k, read, op, arg) in enumerate(cmds):
            g = self.guid.get(_b(k))
            if g is None:
                out["status"][i] = Q_NO_KEY if read else U_NO_KEY
                continue
            out["guid"][i] = g
            if g not in self.reg or (self.reg[g][0] == 1 and not self.orset) or (self.reg[g][0] == 0 and self.P is None):
                out["status"][i] = Q_NO_CRDT if read else U_NO_CRDT
                continue
            t, ix = self.reg[g]
            out["kind"][i] = t
            name = None if arg is self.null else _b(arg) if isinstance(arg, (str, bytes)) else arg
            if read:
                if t == 0:  # PNCounterWrapper.Query never reads args
                    v, o = orc.pnc_values(self.P[ix:ix + 1], self.N[ix:ix + 1])
                    out["status"][i], out["value"][i] = (Q_OVERFLOW, 0) if o[0] else (Q_OK, v[0])
                    out["idx"][i] = ix
                elif arg is None or _is_int(arg):  # ORSetWrapper.Query dereferences args[0]
                    out["status"][i] = Q_NO_ARG
                else:
                    out["value"][i] = 1 if self.sets.get(ix, ORSetStr()).Contains(name) else 0
                    out["idx"][i], out["elem"][i] = ix, self.it.id_of(ix, name)
                continue
            st = write_rule(t, op, arg, self.null)
            out["status"][i] = st
            if st != U_OK:
                continue
            out["idx"][i] = ix
            if t == 0:
                self.P, self.N = orc.pnc_apply_ops(self.P, self.N, [ix], [col], [int(arg)], [op == DEC])
                out["result"][i] = 1
            else:
                nm = None if op == CLEAR else name
                out["result"][i] = 1 if self.sets.setdefault(ix, ORSetStr()).apply(op, nm, (int(lo[i]), int(hi[i]))) else 0
                out["elem"][i] = self.it.op(ix, op, nm)[0]
        return out


__all__ = ["ExecModel", "write_rule", "NULL_ELEM"]
