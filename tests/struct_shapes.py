"""Hand-built Yjs v1 updates whose structs have chosen shapes (test infrastructure): one client
section, struct by struct, with the kind and the byte offset of every struct recorded."""
from tests.histories import any_int, any_str


def vu(v):
    out = bytearray()
    while v > 0x7F:
        out.append(0x80 | (v & 0x7F))
        v >>= 7
    out.append(v)
    return bytes(out)


def vstr(s):
    b = s if isinstance(s, bytes) else s.encode()
    return vu(len(b)) + b


def _obj(*members):
    return bytes([118]) + vu(len(members)) + b"".join(vstr(k) + v for k, v in members)


KINDS = ("deleted", "int", "string", "object", "array", "root_key", "root_id", "gc", "skip", "cstring",
         "binary", "type", "embed", "format", "json", "rorigin")


class Builder:
    """One client's struct section, struct by struct: items appended to the root array `list` by
    origin, map entries of the root map `users` and of a nested YMap (parent by id), GC / Skip."""

    def __init__(self, client, tag):
        self.client, self.tag = client, tag
        self.clock = 0
        self.out = []
        self.last = None   # last clock of the list's last item
        self.first = None  # the list's first item and its successor (a right-origin insert goes between)
        self.second = None
        self.mid = None    # last item typed between them
        self.nested = None  # clock of the nested YMap's ContentType item
        self.n = 0
        self.size = 0
        self.marks = []    # (offset in the struct section, kind as emitted) of every struct
        self.kind = None

    def _emit(self, b, length):
        self.marks.append((self.size, self.kind))
        self.size += len(b)
        self.out.append(b)
        start = self.clock
        self.clock += length
        self.n += 1
        return start

    def _list_item(self, ref, content, length):
        if self.last is None:
            start = self._emit(bytes([ref]) + vu(1) + vstr("list") + content, length)
            self.first = start + length - 1
        else:
            start = self._emit(bytes([ref | 0x80]) + vu(self.client) + vu(self.last) + content, length)
            if self.second is None:
                self.second = start
        self.last = start + length - 1

    def _map_item(self, ref, content, key):
        self._emit(bytes([ref | 0x20]) + vu(1) + vstr("users") + vstr(key) + content, 1)

    def add(self, kind, lazy=False):
        k, t = self.n, self.tag
        if kind == "skip" and not lazy:
            kind = "gc"  # (a Skip inside a section leaves the rest pending: lazy cases only)
        if kind in ("root_id", "rorigin") and (self.nested is None or self.second is None):
            kind = "type" if self.nested is None and kind == "root_id" else "int"
        self.kind = kind
        if kind == "deleted":
            self._list_item(1, vu(3), 3)
        elif kind == "int":
            self._list_item(8, vu(1) + any_int(k * 37 - 500), 1)
        elif kind == "string":
            self._list_item(8, vu(1) + any_str(f"{t}-s{k}"), 1)
        elif kind == "object":
            self._list_item(8, vu(1) + _obj(("name", any_str(f"{t}{k}"))), 1)
        elif kind == "array":
            self._list_item(8, vu(2) + bytes([117]) + vu(2) + any_int(k) + any_str("e") + any_int(-k), 2)
        elif kind == "root_key":
            self._map_item(8, vu(1) + any_int(k), f"k{k}")
        elif kind == "root_id":
            self._emit(bytes([8 | 0x20]) + vu(0) + vu(self.client) + vu(self.nested) + vstr(f"n{k}") + vu(1) + any_str(f"v{k}"), 1)
        elif kind == "gc":
            self._emit(bytes([0]) + vu(2), 2)
        elif kind == "skip":
            self._emit(bytes([10]) + vu(3), 3)
        elif kind == "cstring":
            s = f"hé{k}\U0001F600"
            self._list_item(4, vstr(s), len(s.encode("utf-16-le")) // 2)
        elif kind == "binary":
            self._list_item(3, vstr(bytes([0, 1, 0xFE, 0xFF, k & 0xFF])), 1)
        elif kind == "type":
            if self.nested is None:  # a YMap under users[nested]
                self.nested = self._emit(bytes([7 | 0x20]) + vu(1) + vstr("users") + vstr("nested") + vu(1), 1)
            else:
                self._list_item(7, vu(0), 1)
        elif kind == "embed":
            self._list_item(5, vstr('{"e":%d}' % k), 1)
        elif kind == "format":
            self._list_item(6, vstr("bold") + vstr("true"), 1)
        elif kind == "json":
            self._list_item(2, vu(2) + vstr("%d" % k) + vstr('"j"'), 2)
        elif kind == "rorigin":  # typed between the list's first two items
            o = self.first if self.mid is None else self.mid
            self.mid = self._emit(bytes([8 | 0xC0]) + vu(self.client) + vu(o) + vu(self.client) + vu(self.second) + vu(1) + any_int(k), 1)
        elif kind == "other":  # a key that pushes the content out of the classifier's window
            self._map_item(8, vu(1) + any_str(f"v{k}"), f"a-long-key-of-the-map-{k:05d}")
        elif kind == "nested_any":  # an `any` nested two levels: the deferred list
            self._list_item(8, vu(1) + _obj(("o", _obj(("i", any_int(k)), ("a", bytes([117]) + vu(1) + any_str("x"))))), 1)
        elif kind == "doc":  # ContentDoc: guid + options (deferred too)
            self._list_item(9, vstr(f"guid-{t}-{k}") + _obj(), 1)
        else:
            raise ValueError(kind)

    def header(self):
        return vu(1) + vu(self.n) + vu(self.client) + vu(0)

    def update(self):
        return self.header() + b"".join(self.out) + vu(0)

    def starts(self):
        """(byte offset in update(), kind) of every struct."""
        h = len(self.header())
        return [(h + o, k) for o, k in self.marks]


def one_shape(n, client=7):
    b = Builder(client, "u")
    for _ in range(n):
        b.add("root_key")
    return b.update()


def interleaved(period, n, client, lazy=False, tag="i"):
    b = Builder(client, tag)
    for k in range(n):
        b.add(KINDS[(k % period + period * (k // (8 * period))) % len(KINDS)], lazy)
    return b.update()


def only_other(n, client=21):
    b = Builder(client, "o")
    for _ in range(n):
        b.add("other")
    return b.update()


def with_deferred(n, client=23):
    b = Builder(client, "d")
    for k in range(n):
        b.add("nested_any" if k % 50 == 20 else "doc" if k % 50 == 45 else KINDS[k % 5])
    return b.update()
