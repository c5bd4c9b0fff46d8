"""Restatement of TPSet<string?> (MergeSharp/MergeSharp/CRDTs/2P-Set.cs) and of TPSetMsg's wire codec — the checker
of the device set jg_tpset_* (the set KeySpaceManager keeps its keys in, BFT-CRDT/CRDTManagers/KeySpaceManager.cs:34).

Strings are `bytes` (UTF-8), the C# null element is None.  A HashSet that nothing is removed from enumerates in
first-insertion order: a dict with insertion order stands for it.

Encode: System.Text.Json's compact output, strings escaped by JavaScriptEncoder.Default as oracle/json.hpp:8-13
describes.  Decode: the accept contract at the top of oracle/json.hpp (whitespace between tokens, members in any
order, unknown members skipped with any well-formed value to depth 64, a repeated member's last occurrence wins, full
JSON strings with UTF-8 and surrogates validated, a string repeated inside one array de-duplicated), with the one
rule the key-space set adds: Merge walks addSet before removeSet, so a message whose addSet is valid and whose
removeSet is missing or null applies its addSet and stops the call (`partial`).
"""
from __future__ import annotations

import re

MAX_DEPTH = 64
_TWO = {0x5C: b"\\\\", 0x08: b"\\b", 0x09: b"\\t", 0x0A: b"\\n", 0x0C: b"\\f", 0x0D: b"\\r"}
_U16 = set(b"\"&'+<>`") | {0x7F} | set(range(0x20))
_ASCII = {c: _TWO.get(c) or b"\\u%04X" % c for c in set(_TWO) | _U16}
_RUN = re.compile(rb'[^"\\\x00-\x1f\x80-\xff]*').match
_ASCII_SUB = re.compile(b"[" + b"".join(b"\\x%02x" % c for c in sorted(_ASCII)) + b"]").sub


def escape(s: bytes) -> bytes:
    """JavaScriptEncoder.Default over well-formed UTF-8 (oracle/json.hpp EscapeTo)."""
    if s.isascii():  # the same two tables in one pass: what keeps a large state's encoding quick
        return _ASCII_SUB(lambda m: _ASCII[m.group()[0]], s)
    o = bytearray()
    for ch in s.decode("utf-8"):
        cp = ord(ch)
        if cp < 0x80:
            if cp in _TWO:
                o += _TWO[cp]
            elif cp in _U16:
                o += b"\\u%04X" % cp
            else:
                o.append(cp)
        elif cp >= 0x10000:
            cp -= 0x10000
            o += b"\\u%04X\\u%04X" % (0xD800 | cp >> 10, 0xDC00 | cp & 0x3FF)
        else:
            o += b"\\u%04X" % cp
    return bytes(o)


def encode_msg(add, rem) -> bytes:
    """TPSetMsg.Encode() (2P-Set.cs:49-52): {"addSet":[...],"removeSet":[...]}."""
    def arr(items):
        return b",".join(b"null" if x is None else b'"' + escape(x) + b'"' for x in items)
    return b'{"addSet":[' + arr(add) + b'],"removeSet":[' + arr(rem) + b"]}"


class JsonError(ValueError):
    pass


class _Reader:
    """oracle/json.hpp Reader over bytes."""

    def __init__(self, s: bytes):
        self.s, self.p = s, 0

    def fail(self, what):
        raise JsonError(f"{what} at byte {self.p}")

    def ws(self):
        while self.p < len(self.s) and self.s[self.p] in b" \t\n\r":
            self.p += 1

    def peek(self):
        self.ws()
        return self.s[self.p] if self.p < len(self.s) else -1

    def expect(self, c: bytes):
        if self.peek() != c[0]:
            self.fail("unexpected token")
        self.p += 1

    def eat(self, c: bytes) -> bool:
        if self.peek() == c[0]:
            self.p += 1
            return True
        return False

    def literal(self, lit: bytes):
        if self.s[self.p:self.p + len(lit)] != lit:
            self.fail("bad literal")
        self.p += len(lit)

    def hex4(self) -> int:
        h = self.s[self.p:self.p + 4]
        if len(h) != 4 or any(c not in b"0123456789abcdefABCDEF" for c in h):
            self.fail("bad \\u escape")
        self.p += 4
        return int(h, 16)

    def string(self) -> bytes:
        self.expect(b'"')
        s, o = self.s, bytearray()
        while True:
            run = _RUN(s, self.p).end()  # ASCII that stands for itself, in one step
            o += s[self.p:run]
            self.p = run
            if self.p >= len(s):
                self.fail("unterminated string")
            c = s[self.p]
            self.p += 1
            if c == 0x22:
                return bytes(o)
            if c < 0x20:
                self.fail("control character in string")
            if c == 0x5C:
                if self.p >= len(s):
                    self.fail("bad escape")
                e = s[self.p]
                self.p += 1
                simple = {0x22: 0x22, 0x5C: 0x5C, 0x2F: 0x2F, 0x62: 8, 0x66: 12, 0x6E: 10, 0x72: 13, 0x74: 9}
                if e in simple:
                    o.append(simple[e])
                elif e == 0x75:
                    u = self.hex4()
                    if 0xDC00 <= u <= 0xDFFF:
                        self.fail("lone low surrogate")
                    if 0xD800 <= u <= 0xDBFF:
                        if s[self.p:self.p + 2] != b"\\u":
                            self.fail("lone high surrogate")
                        self.p += 2
                        lo = self.hex4()
                        if not 0xDC00 <= lo <= 0xDFFF:
                            self.fail("bad surrogate pair")
                        u = 0x10000 + ((u - 0xD800) << 10) + (lo - 0xDC00)
                    o += chr(u).encode("utf-8")
                else:
                    self.fail("bad escape")
                continue
            if c < 0x80:
                o.append(c)
                continue
            if 0xC2 <= c <= 0xDF:
                n, cp = 2, c & 0x1F
            elif 0xE0 <= c <= 0xEF:
                n, cp = 3, c & 0x0F
            elif 0xF0 <= c <= 0xF4:
                n, cp = 4, c & 0x07
            else:
                self.fail("invalid UTF-8")
            tail = s[self.p:self.p + n - 1]
            if len(tail) != n - 1 or any(t & 0xC0 != 0x80 for t in tail):
                self.fail("invalid UTF-8")
            for t in tail:
                cp = cp << 6 | (t & 0x3F)
            if (n == 3 and (cp < 0x800 or 0xD800 <= cp <= 0xDFFF)) or (n == 4 and (cp < 0x10000 or cp > 0x10FFFF)):
                self.fail("invalid UTF-8")
            o.append(c)
            o += tail
            self.p += n - 1

    def skip_value(self, depth: int):
        c = self.peek()
        if c == -1:
            self.fail("unexpected end")
        if c in b"{[":
            if depth + 1 > MAX_DEPTH:
                self.fail("depth past MaxDepth")
            self.p += 1
            close = b"}" if c == 0x7B else b"]"
            if self.eat(close):
                return
            while True:
                if c == 0x7B:
                    self.string()
                    self.expect(b":")
                self.skip_value(depth + 1)
                if not self.eat(b","):
                    break
            self.expect(close)
            return
        if c == 0x22:
            self.string()
            return
        for lit in (b"true", b"false", b"null"):
            if self.s[self.p:self.p + len(lit)] == lit:
                self.p += len(lit)
                return
        m = re.compile(rb"-?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)?").match(self.s, self.p)
        if not m:
            self.fail("not a value")
        self.p = m.end()
        if self.p < len(self.s) and self.s[self.p] in b"0123456789.eE+-":
            self.fail("bad number")


def decode_msg(msg: bytes):
    """-> (add, rem): lists of bytes | None in array order, duplicates kept; a member that is missing or whose last
    occurrence is null comes back as None.  JsonError when the message is malformed."""
    r = _Reader(msg)
    val = {"addSet": None, "removeSet": None}
    r.expect(b"{")
    if r.peek() != 0x7D:
        while True:
            name = r.string()
            r.expect(b":")
            key = {b"addSet": "addSet", b"removeSet": "removeSet"}.get(name)
            if key is None:
                r.skip_value(1)
            elif r.peek() == 0x6E:
                r.literal(b"null")
                val[key] = None
            else:
                items = []
                r.expect(b"[")
                if not r.eat(b"]"):
                    while True:
                        c = r.peek()
                        if c == 0x22:
                            items.append(r.string())
                        elif c == 0x6E:
                            r.literal(b"null")
                            items.append(None)
                        else:
                            r.fail("not a string")
                        if not r.eat(b","):
                            break
                    r.expect(b"]")
                val[key] = items
            if not r.eat(b","):
                break
    r.expect(b"}")
    r.ws()
    if r.p != len(msg):
        r.fail("trailing data")
    return val["addSet"], val["removeSet"]


class TPSetRef:
    """TPSet<string?>: two insertion-ordered sets."""

    def __init__(self):
        self.add_set: dict = {}
        self.rem_set: dict = {}

    def add(self, x):  # 2P-Set.cs:106-109
        self.add_set.setdefault(x, None)

    def contains(self, x) -> bool:  # :169-172
        return x in self.add_set and x not in self.rem_set

    def remove(self, x) -> bool:  # :117-126
        if self.contains(x):
            self.rem_set.setdefault(x, None)
            return True
        return False

    def apply_ops(self, ops):
        out = []
        for op, x in ops:
            if op == 1:
                self.add(x)
                out.append(True)
            else:
                out.append(self.remove(x))
        return out

    def count(self) -> int:  # :76-82
        return len(self.add_set) - len(self.rem_set)

    def lookup_all(self, from_ord: int = 0, with_ords: bool = False):  # :133-136
        out = [(i, x) for i, x in enumerate(self.add_set) if i >= from_ord and x not in self.rem_set]
        return out if with_ords else [x for _, x in out]

    def merge(self, add, rem):  # :188-192
        for x in add:
            self.add_set.setdefault(x, None)
        for x in rem:
            self.rem_set.setdefault(x, None)

    def size(self):
        return (len(self.add_set), len(self.rem_set),
                sum(len(x) for x in set(self.add_set) | set(self.rem_set) if x is not None))

    def encode(self) -> bytes:  # GetLastSynchronizedUpdate().Encode(), :210-213
        return encode_msg(list(self.add_set), list(self.rem_set))

    def merge_json(self, msgs):
        """Message after message; -> (bad_msg | None, partial).  Every message before the first bad one is applied,
        nothing after it; a bad message with a valid addSet and no removeSet has its addSet applied (partial)."""
        for i, m in enumerate(msgs):
            try:
                add, rem = decode_msg(m)
            except JsonError:
                return i, False
            if add is None:
                return i, False
            if rem is None:
                self.merge(add, [])
                return i, True
            self.merge(add, rem)
        return None, False


# ---- KeySpaceManager (BFT-CRDT/CRDTManagers/KeySpaceManager.cs) -------------------------------------------------
def guid_d(g) -> bytes:
    """Guid.ToString() ("D", lower case) of (lo, hi): bytes b0..b15 print as b3b2b1b0-b5b4-b7b6-b8b9-b10..b15."""
    b = g[0].to_bytes(8, "little") + g[1].to_bytes(8, "little")
    order = [3, 2, 1, 0, 5, 4, 7, 6, 8, 9, 10, 11, 12, 13, 14, 15]
    h = "".join("%02x" % b[i] for i in order)
    return ("%s-%s-%s-%s-%s" % (h[:8], h[8:12], h[12:16], h[16:20], h[20:])).encode()


def parse_guid_d(s: bytes):
    """The "D" form of either case -> (lo, hi), or None."""
    if len(s) != 36 or any(s[i] != 0x2D for i in (8, 13, 18, 23)):
        return None
    h = s[:8] + s[9:13] + s[14:18] + s[19:23] + s[24:]
    if any(c not in b"0123456789abcdefABCDEF" for c in h):
        return None
    t = bytes.fromhex(h.decode())
    order = [3, 2, 1, 0, 5, 4, 7, 6, 8, 9, 10, 11, 12, 13, 14, 15]
    b = bytearray(16)
    for i, o in enumerate(order):
        b[o] = t[i]
    return int.from_bytes(b[:8], "little"), int.from_bytes(b[8:], "little")


class KeySpaceRef:
    """The key-space CRDT, keySpaces and LastKeySpaceSet, with OnNext (:151-178) run after every merged message.
    In the reference's order: the null element first (it is dereferenced before any lookup), then ContainsKey of the
    bytes before the first NUL (the whole entry if it has none) - an entry of a key the dictionary holds is skipped
    whatever the rest of it looks like - and only then Split(...)[1] and Guid.Parse.
    Stated departure from the reference, which throws out of OnNext (and so wedges) on such entries: an entry of an
    unknown key without a NUL (status 1) or with a guid segment not in "D" form (2), and the null element (3), is
    journalled with its raw bytes, not added, and processing goes on."""

    def __init__(self):
        self.set = TPSetRef()
        self.keys: dict = {}
        self.last: set = set()
        self.journal: list = []

    def create_keys(self, pairs):  # CreateNewKVPair :121-136
        out = []
        for key, guid in pairs:
            out.append(key not in self.keys)
            self.keys.setdefault(key, guid)  # TryAdd
            self.set.add(key + b"\0" + guid_d(guid))
        return out

    def on_next(self):
        now = self.set.lookup_all()
        for x in now:
            if x in self.last:
                continue
            if x is None:
                self.journal.append((b"", (0, 0), 3))
                continue
            parts = x.split(b"\0")
            if parts[0] in self.keys:  # :164 ContainsKey comes first: Split(...)[1] and Guid.Parse never run
                continue
            if len(parts) < 2:
                self.journal.append((x, (0, 0), 1))
                continue
            guid = parse_guid_d(parts[1])
            if guid is None:
                self.journal.append((x, (0, 0), 2))
            else:
                self.keys[parts[0]] = guid
                self.journal.append((parts[0], guid, 0))
        self.last = set(now)

    def receive(self, msgs):
        """-> (bad_msg | None, partial): Merge then OnNext per message; a rejected message stops the call before its OnNext."""
        for i, m in enumerate(msgs):
            bad, partial = self.set.merge_json([m])
            if bad is not None:
                return i, partial
            self.on_next()
        return None, False
