"""yc_write.h on the host: the two update writers the fleet-write kernels (yc_write.hip,
ycrdt_docs_write) run one lane per op — the one-item update (Item.write between the update's header
and an empty delete set) and the delete-set-only update (ranges sorted by client and clock, adjacent
ones merged, grouped per client). tests/csrc/write_bytes_main.cpp sizes every case, writes it into a
heap block of exactly that size under AddressSanitizer and UBSan and compares it with the bytes built
here from tests/v1util.py's varUint writer, following Yjs 13.5.16's Item.write and writeDeleteSet."""
import itertools
import os
import subprocess

from tests import v1util

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WRITE_RANGES_MAX = 8

CLIENTS = (0, 127, 128, 0xFFFFFFFF)
CLOCKS = (0, 127, 128, 16383, 16384)


def vu(n):
    out = bytearray()
    v1util.wvu(out, n)
    return bytes(out)


def vs(b):
    return vu(len(b)) + b


def item_update(client, clock, ref, origin, right, parent, root, key, lead, content):
    """parent: an item id or None (the root type `root`); key: bytes or None."""
    info = ref | (0x80 if origin else 0) | (0x40 if right else 0) | (0x20 if key is not None else 0)
    out = vu(1) + vu(1) + vu(client) + vu(clock) + bytes([info])
    for i in (origin, right):
        if i:
            out += vu(i[0]) + vu(i[1])
    if not origin and not right:
        out += (vu(0) + vu(parent[0]) + vu(parent[1])) if parent else (vu(1) + vs(root))
        if key is not None:
            out += vs(key)
    return out + vu(lead) + content + vu(0)


def ds_update(ranges):
    merged = []
    for c, k, n in sorted(ranges):
        if merged and merged[-1][0] == c and merged[-1][1] + merged[-1][2] == k:
            merged[-1][2] += n
        else:
            merged.append([c, k, n])
    out = vu(0)
    clients = list(dict.fromkeys(c for c, _, _ in merged))
    out += vu(len(clients))
    for c in clients:
        rs = [(k, n) for cc, k, n in merged if cc == c]
        out += vu(c) + vu(len(rs)) + b"".join(vu(k) + vu(n) for k, n in rs)
    return out


def hx(b):
    return b.hex() or "-"


def item_line(client, clock, ref, origin, right, parent, root, key, lead, content):
    want = item_update(client, clock, ref, origin, right, parent, root, key, lead, content)
    o, r, p = origin or (0, 0), right or (0, 0), parent or (0, 0)
    return (f"I {client} {clock} {ref} {int(bool(origin))} {o[0]} {o[1]} {int(bool(right))} {r[0]} {r[1]} {int(bool(parent))} {p[0]} {p[1]} "
            f"{int(key is not None)} {hx(root)} {hx(key or b'')} {lead} {hx(content)} {hx(want)}"), want


def ds_line(ranges):
    want = ds_update(ranges)
    return f"D {len(ranges)} " + " ".join(f"{c} {k} {n}" for c, k, n in ranges) + f" {hx(want)}", want


def _run(tmp_path, lines):
    exe = tmp_path / "write_bytes"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "crdt_amd", "csrc"), os.path.join(HERE, "csrc", "write_bytes_main.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    out = r.stdout.splitlines()
    assert out[-1] == f"OK {len(lines)} cases" and not any(x.startswith("FAIL") for x in out), out[-20:]
    return out[:-1]


def test_item_updates(tmp_path):
    lines, wants = [], []
    # every combination of origin / right origin / parent kind / key, over the id edges
    ids = list(itertools.product(CLIENTS, CLOCKS))
    for k, (ho, hr, pi, hk) in enumerate(itertools.product((0, 1), repeat=4)):
        for j, (client, clock) in enumerate(ids):
            oc, ok = ids[(j + 3 * k + 1) % len(ids)]
            rc, rk = ids[(j + 5 * k + 7) % len(ids)]
            pc, pk = ids[(j + 11) % len(ids)]
            line, want = item_line(client, clock, 8 if k % 2 else 7, (oc, ok) if ho else None, (rc, rk) if hr else None,
                                   (pc, pk) if pi else None, b"users", b"k\xc3\xa9y" if hk else None, 1 + j % 3, bytes([125, j % 64]) * (1 + j % 3))
            lines.append(line)
            wants.append(want)
    # an empty root name and an empty key; a long root, key and content; no content behind the lead (a type ref)
    for root, key, lead, content in ((b"", b"", 1, bytes([125, 1])), (b"", None, 1, bytes([127])), (b"r", b"", 0, b""),
                                    (b"R" * 200, b"K" * 64, 300, bytes([119, 2, 104, 105]) * 300), (b"m", b"k", 1, b"")):
        line, want = item_line(5, 9, 8, None, None, None, root, key, lead, content)
        lines.append(line)
        wants.append(want)
    out = _run(tmp_path, lines)
    assert [x.split() for x in out] == [["ok", str(len(w))] for w in wants]  # the sizing call equals the written length
    assert len(lines) == 16 * 20 + 5


def test_delete_set_updates(tmp_path):
    cases = [
        [(5, 3, 2)],                                    # one range
        [(0xFFFFFFFF, 16384, 128)],
        [(9, 0, 1), (5, 7, 2)],                         # two clients given in descending order
        [(5, 4, 2), (5, 6, 3)],                         # one client, adjacent in clock: they merge
        [(5, 6, 3), (5, 4, 2)],                         # ... given the other way round
        [(5, 4, 2), (5, 7, 3)],                         # one client, a gap: they do not merge
        [(5, 7, 3), (5, 4, 2)],
        [(8 - i, 10 * i, i + 1) for i in range(WRITE_RANGES_MAX)],            # WRITE_RANGES_MAX ranges, every client its own
        [(7, 100 - 10 * i, 10) for i in range(WRITE_RANGES_MAX)],             # ... of one client, all adjacent, descending
        [(i % 2, 127 + 2 * (i // 2), 1 + i % 2) for i in range(WRITE_RANGES_MAX)],  # ... two clients, some adjacent
        [],
    ]
    lines, wants = zip(*(ds_line(c) for c in cases))
    assert wants[3] == wants[4] == bytes([0, 1, 5, 1, 4, 5]) and wants[5] == wants[6] == bytes([0, 1, 5, 2, 4, 2, 7, 3])
    assert wants[2] == bytes([0, 2, 5, 1, 7, 2, 9, 1, 0, 1])
    out = _run(tmp_path, list(lines))
    assert [x.split() for x in out] == [["ok", str(len(w))] for w in wants]
