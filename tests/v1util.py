"""Yjs v1 helpers for tests: canonical (13.6) client order of delete sets / state vectors.
Mirrors tests/golden/gen/v1.js canonicalUpdate / canonicalSv."""
from oracle.ymerge import GC, SKIP, Dec, lazy_structs, read_content, wvu


def _skip_structs(d):
    lazy_structs(d)


def canonical_update(u):
    d = Dec(bytes(u))
    _skip_structs(d)
    end = d.p
    ds = []
    for _ in range(d.vu()):
        client = d.vu()
        ranges = [(d.vu(), d.vu()) for _ in range(d.vu())]
        ds.append((client, ranges))
    if d.p != len(u):
        raise ValueError("trailing bytes")
    ds.sort(key=lambda e: -e[0])
    out = bytearray(u[:end])
    wvu(out, len(ds))
    for client, ranges in ds:
        wvu(out, client)
        wvu(out, len(ranges))
        for c, n in ranges:
            wvu(out, c)
            wvu(out, n)
    return bytes(out)


def delete_set_of(u):
    """The delete set of a v1 update as {client: [(clock, len), ...]}: sorted and merged (Yjs
    sortAndMergeDeleteSet, Y@10246), so byte layouts that mean the same deletions compare equal."""
    d = Dec(bytes(u))
    _skip_structs(d)
    ds = {}
    for _ in range(d.vu()):
        client = d.vu()
        for _ in range(d.vu()):
            c, n = d.vu(), d.vu()
            if n:
                ds.setdefault(client, []).append((c, n))
    out = {}
    for client, rs in ds.items():
        rs.sort()
        m = []
        for c, n in rs:
            if m and m[-1][0] + m[-1][1] >= c:
                m[-1] = (m[-1][0], max(m[-1][0] + m[-1][1], c + n) - m[-1][0])
            else:
                m.append((c, n))
        out[client] = m
    return out


def coalesce_gc(u):
    """The update with adjacent GC structs of one client merged where their clocks are contiguous;
    every other struct, the client order and the delete-set bytes stay as they are. Yjs cuts the GC
    structs below a deleted type by the order its applyUpdate calls came in (it re-merges only what a
    transaction touched); this form is the same for every order."""
    u = bytes(u)
    d = Dec(u)
    out = bytearray()
    nsec = d.vu()
    wvu(out, nsec)
    for _ in range(nsec):
        n, client, clock = d.vu(), d.vu(), d.vu()
        structs = []  # raw bytes of a struct as they stand, or the length of a GC run
        for _ in range(n):
            start = d.p
            info = d.u8()
            if info & 31 == GC:
                ln = d.vu()
                if structs and isinstance(structs[-1], int):
                    structs[-1] += ln
                else:
                    structs.append(ln)
                continue
            if info & 31 == SKIP:
                d.vu()
            else:
                # not through Struct.write: it restates an item's info byte (Yjs sets the parentSub
                # bit beside an origin, a lazily read struct has lost it)
                for bit in (0x80, 0x40):
                    if info & bit:
                        d.vu(), d.vu()
                if not info & 0xC0:
                    if d.vu() == 1:
                        d.vstr_raw()
                    else:
                        d.vu(), d.vu()
                    if info & 0x20:
                        d.vstr_raw()
                read_content(d, info)
            structs.append(u[start:d.p])
        wvu(out, len(structs))
        wvu(out, client)
        wvu(out, clock)
        for s in structs:
            if isinstance(s, int):
                out.append(GC)
                wvu(out, s)
            else:
                out += s
    return bytes(out) + u[d.p:]


def canonical_sv(sv):
    """The state vector with its clients in descending order (tests/golden/gen/v1.js canonicalSv)."""
    d = Dec(bytes(sv))
    e = sorted(((d.vu(), d.vu()) for _ in range(d.vu())), key=lambda t: -t[0])
    out = bytearray()
    wvu(out, len(e))
    for c, k in e:
        wvu(out, c)
        wvu(out, k)
    return bytes(out)
