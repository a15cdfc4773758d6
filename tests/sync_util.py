"""Helpers of the sync-reply tests: a v1 update's client blocks with every struct's byte position,
and a reply assembled from a state's own bytes the way ycrdt_docs_diff assembles it (a new header,
the cut struct re-encoded, everything else copied) — on the CPU, from oracle/ymerge.py's readers."""
import json
import os

from oracle.ymerge import GC, ITEM, Dec, Struct, read_content, wvu

HERE = os.path.dirname(os.path.abspath(__file__))


def load_cases(name):
    with open(os.path.join(HERE, "golden", f"{name}.json")) as f:
        return json.load(f)["cases"]


def parse_sv(sv):
    d = Dec(bytes(sv))
    return {c: k for c, k in ((d.vu(), d.vu()) for _ in range(d.vu()))} if sv else {}


def _read_struct(d, client, clock):
    info = d.u8()
    ref = info & 31
    if ref == 0:
        return Struct(GC, client, clock, d.vu())
    origin = (d.vu(), d.vu()) if info & 0x80 else None
    right = (d.vu(), d.vu()) if info & 0x40 else None
    parent = psub = None
    if (info & 0xC0) == 0:
        parent = d.vstr_raw() if d.vu() == 1 else (d.vu(), d.vu())
        if info & 0x20:
            psub = d.vstr_raw()
    elif info & 0x20:
        psub = b""  # (the bit without the string: an item with an origin under a map key)
    ln, content = read_content(d, info)
    return Struct(ITEM, client, clock, ln, ref, origin, right, parent, psub, content)


def blocks(u):
    """([block], delete-set start): block = dict(client, clock, n, hdr, first, end, structs=[(pos, Struct)])."""
    u = bytes(u)
    d = Dec(u)
    out = []
    for _ in range(d.vu()):
        hdr = d.p
        n, client, clock = d.vu(), d.vu(), d.vu()
        b = dict(client=client, clock=clock, n=n, hdr=hdr, first=d.p, structs=[])
        for _ in range(n):
            pos = d.p
            s = _read_struct(d, client, clock)
            b["structs"].append((pos, s))
            clock += s.length
        b["end"] = d.p
        b["end_clock"] = clock
        out.append(b)
    return out, d.p


def reply_from_state(state, sv):
    """Y.encodeStateAsUpdate(doc, sv) from the doc's canonical state bytes alone."""
    state = bytes(state)
    want = parse_sv(sv)
    bl, ds = blocks(state)
    parts = []
    for b in bl:
        svc = want.get(b["client"], 0)
        if svc >= b["end_clock"]:
            continue
        if svc <= b["clock"]:
            parts.append(state[b["hdr"]:b["end"]])
            continue
        k = max(i for i, (_, s) in enumerate(b["structs"]) if s.clock <= svc)
        pos, s = b["structs"][k]
        out = bytearray()
        wvu(out, b["n"] - k)
        wvu(out, b["client"])
        wvu(out, svc)
        if svc > s.clock:
            s.write(out, svc - s.clock)
            tail = b["structs"][k + 1][0] if k + 1 < b["n"] else b["end"]
        else:
            tail = pos
        parts.append(bytes(out) + state[tail:b["end"]])
    head = bytearray()
    wvu(head, len(parts))
    return bytes(head) + b"".join(parts) + state[ds:]
