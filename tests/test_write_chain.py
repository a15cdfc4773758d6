"""The transaction planner (ycrdt_docs_transact) on the CPU.

crdt_amd/csrc/yc_write.h plans a list op behind the earlier ops of its call on the same list over a
small piece table (write_list_plan), and crdt_amd/csrc/yc_engine_host.h finds how a document's ops
depend on one another (transact_links). tests/csrc/write_chain_main.cpp runs both as a stand-alone
program, built with AddressSanitizer and UBSan.

Expected plans come from oracle/yref.py's Doc: the list is built with apply_update, the same ops run
one by one, and each op's origin, right origin and delete ranges are read off its effect on
encode_state_as_update. The planner sees only the list BEFORE the chain and the ops."""
import json
import os
import random
import subprocess

import pytest

from oracle.yref import Doc, OracleError
from oracle.ymerge import ITEM, Dec, decode_sv, lazy_structs
from tests import v1util

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INSERT, PUSH, DELETE = 3, 4, 5
WHY_NO_TYPE, WHY_MISMATCH, WHY_LENGTH = 1, 2, 3
WF_RANGES, WF_PIECES = 32, 64
OWN = 1000
ANY1 = bytes([125, 1])


def vu(n):
    out = bytearray()
    v1util.wvu(out, n)
    return bytes(out)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("write_chain") / "write_chain")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "crdt_amd", "csrc"),
                           os.path.join(HERE, "csrc", "write_chain_main.cpp"), "-o", path])
    return path


def _run(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    out = r.stdout.splitlines()
    assert out[-1] == f"OK {len(lines)} cases" and not any(x.startswith("FAIL") for x in out), out[-5:]
    flagged = tuple(int(x) for x in out[-2].split()[1:])
    return out[:-2], flagged


# ---------------------------------------------------------------- the oracle's side
def _deleted_ids(doc):
    ds = v1util.delete_set_of(doc.encode_state_as_update())
    return {(c, k + i) for c, rs in ds.items() for k, n in rs for i in range(n)}


def _oracle_op(doc, own, root, op, values=None):
    """Runs (kind, index, length, count) on the oracle. Returns the clock the op's item takes and what
    the op did: ("item", origin, right) | ("ranges", {ids}) | ("nothing",), and whether it failed."""
    kind, index, length, count = op
    sv = doc.encode_state_vector()
    clock = decode_sv(sv).get(own, 0)
    dead = _deleted_ids(doc)
    failed = False
    try:
        if kind == DELETE:
            doc.array_delete(root, index, length)
        else:
            if kind == PUSH:
                index = len(json.loads(doc.root_json(root, "array")))
            doc.array_insert(root, index, values if values is not None else [ANY1] * count)
    except OracleError:
        failed = True
    mine = [s for s in lazy_structs(Dec(doc.encode_state_as_update(sv))) if s.client == own and s.kind == ITEM]
    gone = _deleted_ids(doc) - dead
    assert not (mine and gone)
    if mine:
        assert mine[0].clock == clock and sum(s.length for s in mine) == count and not failed
        return clock, ("item", mine[0].origin, mine[0].right_origin), failed
    if gone:
        return clock, ("ranges", gone), failed
    return clock, ("nothing",), failed


def _check_plans(got, want):
    """got: the program's P lines of one chain; want: [(effect, failed)]. Returns the flagged ops."""
    flagged = 0
    assert len(got) == len(want)
    for g, (effect, failed) in zip(got, want):
        f = g.split()
        assert f[0] == "P"
        kind, has, oc, ok, rc, rk, why, flags, nr = (int(x) for x in f[1:10])
        if flags:
            assert flags in (WF_RANGES, WF_PIECES), g
            flagged += 1
            continue
        assert why == (WHY_LENGTH if failed else 0), (g, effect, failed)
        if effect[0] == "item":
            assert kind == 1, (g, effect)
            assert ((oc, ok) if has & 1 else None) == effect[1], (g, effect)
            assert ((rc, rk) if has & 2 else None) == effect[2], (g, effect)
        elif effect[0] == "ranges":
            assert kind == 2 and nr >= 1, (g, effect)
            r = [int(x) for x in f[10:]]
            ranges = [tuple(r[3 * i:3 * i + 3]) for i in range(nr)]
            assert ranges == sorted(ranges)
            for (c0, k0, n0), (c1, k1, _) in zip(ranges, ranges[1:]):
                assert c0 != c1 or k0 + n0 < k1, g  # merged
            ids = [(c, k + i) for c, k, n in ranges for i in range(n)]
            assert len(ids) == len(set(ids)) and set(ids) == effect[1], (g, effect)
        else:
            assert kind == 0, (g, effect)
    return flagged


# ---------------------------------------------------------------- seeded chains over hand-built lists
def _list_updates(segs, root="l"):
    """segs: (client, clock, len, visible) in list order, every one behind the last element of the one
    before it; one update per segment and one delete set."""
    ups = []
    prev = None
    for client, clock, n, _ in segs:
        body = bytes([8 | (0x80 if prev else 0)]) + (vu(prev[0]) + vu(prev[1]) if prev else vu(1) + vu(len(root)) + root.encode())
        body += vu(n) + ANY1 * n
        ups.append(vu(1) + vu(1) + vu(client) + vu(clock) + body + vu(0))
        prev = (client, clock + n - 1)
    dead = [(c, k, n) for c, k, n, v in segs if not v]
    if dead:
        clients = sorted({c for c, _, _ in dead})
        ds = vu(len(clients))
        for c in clients:
            rs = [(k, n) for cc, k, n in dead if cc == c]
            ds += vu(c) + vu(len(rs)) + b"".join(vu(k) + vu(n) for k, n in rs)
        ups.append(vu(0) + ds)
    return ups


def _random_segs(rnd):
    segs, clock = [], {5: 0, 9: 0}
    shape = rnd.choice(("plain", "dead head", "dead tail", "alternate", "random"))
    n = rnd.randint(0, 9)
    for i in range(n):
        c = rnd.choice((5, 9))
        ln = rnd.randint(1, 3)
        if shape == "plain":
            vis = 1
        elif shape == "dead head":
            vis = int(i > 0)
        elif shape == "dead tail":
            vis = int(i < n - 1)
        elif shape == "alternate":
            vis = i % 2
        else:
            vis = rnd.randint(0, 1)
        segs.append((c, clock[c], ln, vis))
        clock[c] += ln
    return segs


def _random_chain(rnd, length_now):
    """1-8 ops, drawn around the list's length as it develops (a model of the length only)."""
    ops = []
    ln = length_now
    for _ in range(rnd.randint(1, 8)):
        what = rnd.random()
        if what < 0.15:
            count = rnd.choice((1, 1, 2, 3, 0))
            ops.append((PUSH, 0, 0, count))
            ln += count
        elif what < 0.6:
            count = rnd.choice((1, 1, 2, 3, 0))
            index = rnd.choice((0, ln, max(ln - 1, 0), rnd.randint(0, ln), rnd.randint(0, ln), ln + 1 if rnd.random() < 0.2 else 0))
            ops.append((INSERT, index, 0, count))
            if index <= ln:
                ln += count
        else:
            index = rnd.choice((0, rnd.randint(0, ln), rnd.randint(0, ln), ln, ln + 2))
            length = rnd.choice((0, 1, 1, 2, 3, ln, ln + 3))
            ops.append((DELETE, index, length, 0))
            ln -= max(0, min(ln, index + length) - min(ln, index))
    return ops


def _chain_case(segs, ops, own=OWN, root="l", doc=None):
    """The program's line for the chain, and what the oracle does with it."""
    if doc is None:
        doc = Doc(own)
        for u in _list_updates(segs, root):
            doc.apply_update(u)
    want, fields = [], []
    for op in ops:
        clock, effect, failed = _oracle_op(doc, own, root, op)
        want.append((effect, failed))
        fields.append(f"{op[0]} {op[1]} {op[2]} {op[3]} {clock}")
    line = f"L {own} {len(segs)} " + " ".join(f"{c} {k} {n} {v}" for c, k, n, v in segs) + f" {len(ops)} " + " ".join(fields)
    return " ".join(line.split()), want


HAND = [
    # (segments, ops): the shapes the rules of §5.2h are there for
    ([(5, 0, 2, 1), (5, 2, 1, 0), (5, 3, 1, 1)], [(INSERT, 2, 0, 1), (INSERT, 2, 0, 1), (INSERT, 3, 0, 2), (INSERT, 4, 0, 1)]),  # behind a view element a deleted segment follows, twice; inside and behind the runs
    ([(5, 0, 1, 0), (5, 1, 2, 1)], [(INSERT, 0, 0, 1), (INSERT, 0, 0, 1), (INSERT, 0, 0, 1)]),       # at 0 three times, a deleted head
    ([(5, 0, 1, 0)], [(PUSH, 0, 0, 2), (PUSH, 0, 0, 1), (INSERT, 0, 0, 1), (DELETE, 0, 9, 0)]),      # nothing visible, a deleted segment
    ([], [(PUSH, 0, 0, 1), (PUSH, 0, 0, 1), (DELETE, 0, 1, 0), (DELETE, 0, 1, 0), (DELETE, 0, 1, 0)]),  # an empty list; a delete of nothing
    ([(5, 0, 3, 1), (9, 0, 2, 1)], [(INSERT, 3, 0, 3), (INSERT, 5, 0, 1), (DELETE, 2, 5, 0), (DELETE, 1, 1, 0), (PUSH, 0, 0, 1)]),  # a run cut by an insert, a delete across view, runs, view
    ([(5, 0, 3, 1)], [(DELETE, 1, 1, 0), (INSERT, 1, 0, 1), (DELETE, 0, 3, 0), (DELETE, 0, 3, 0), (PUSH, 0, 0, 1)]),  # dead pieces stay in place
    ([(5, 0, 2, 1), (9, 0, 2, 0), (5, 2, 2, 1)], [(DELETE, 1, 2, 0), (INSERT, 1, 0, 1), (INSERT, 2, 0, 1), (DELETE, 0, 9, 0)]),
    ([(5, 0, 4, 1)], [(INSERT, 9, 0, 1), (DELETE, 9, 1, 0), (DELETE, 3, 4, 0), (INSERT, 3, 0, 1), (INSERT, 4, 0, 1)]),  # failing ops leave nothing behind
]


def test_seeded_chains(exe):
    rnd = random.Random(20241)
    lines, wants = [], []
    for segs, ops in HAND:
        line, want = _chain_case(segs, ops)
        lines.append(line)
        wants.append(want)
    for _ in range(400):
        segs = _random_segs(rnd)
        ops = _random_chain(rnd, sum(n for _, _, n, v in segs if v))
        line, want = _chain_case(segs, ops)
        lines.append(line)
        wants.append(want)
    out, (f_ranges, f_pieces, f_other) = _run(exe, lines)
    at = flagged = 0
    seen = {"item": 0, "ranges": 0, "nothing": 0, "failed": 0}
    for want in wants:
        flagged += _check_plans(out[at:at + len(want)], want)
        at += len(want)
        for effect, failed in want:
            seen[effect[0]] += 1
            seen["failed"] += failed
    assert at == len(out)
    print(f"{len(lines)} chains, {at} ops, {seen}; flagged: ranges {f_ranges}, pieces {f_pieces}, other {f_other}")
    assert f_other == 0 and flagged == f_ranges + f_pieces
    assert f_pieces == 0  # at most 7 earlier ops: 1 + 2 * 7 pieces
    assert min(seen.values()) >= 50, seen


# ---------------------------------------------------------------- Yjs's recorded scripts
def _list_segments(state, root):
    """The root list `root` of a document state as (client, clock, len, visible) segments in list
    order: the items integrated as Yjs does (Item.integrate, Y@82390), one element at a time, and cut
    where the state's structs are cut."""
    d = Dec(bytes(state))
    structs = [s for s in lazy_structs(d) if s.kind == ITEM]
    dead = {(c, k + i) for c, rs in v1util.delete_set_of(state).items() for k, n in rs for i in range(n)}
    name = vu(len(root)) + root.encode()
    member = {}   # element id -> in the list
    todo = []
    for s in structs:
        for i in range(s.length):
            origin = s.origin if i == 0 else (s.client, s.clock + i - 1)
            todo.append(((s.client, s.clock + i), origin, s.right_origin, s, i))
    order = []    # (id, origin, right, struct)
    at = {}
    progress = True
    while todo and progress:
        progress = False
        rest = []
        for el in todo:
            eid, origin, right, s, i = el
            if any(x is not None and x not in member for x in (origin, right)):
                rest.append(el)
                continue
            progress = True
            if origin is not None or right is not None:
                inside = member[origin if origin is not None else right]
            else:
                inside = s.parent == name and s.parent_sub is None
            member[eid] = inside
            if not inside:
                continue
            pos = {x[0]: k for k, x in enumerate(order)}
            left = pos[origin] if origin is not None else -1
            stop = pos[right] if right is not None else len(order)
            before, conflicting = set(), set()
            k = left + 1
            while k < len(order) and k != stop:
                oid, oorigin, oright, _ = order[k]
                before.add(oid)
                conflicting.add(oid)
                if oorigin == origin:
                    if oid[0] < eid[0]:
                        left = k
                        conflicting.clear()
                    elif oright == right:
                        break
                elif oorigin is not None and oorigin in before:
                    if oorigin not in conflicting:
                        left = k
                        conflicting.clear()
                else:
                    break
                k += 1
            order.insert(left + 1, (eid, origin, right, s))
        todo = rest
    assert not todo
    segs = []
    for (c, k), _, _, s in order:
        vis = int((c, k) not in dead)
        if segs and segs[-1][4] is s and segs[-1][0] == c and segs[-1][1] + segs[-1][2] == k and segs[-1][3] == vis:
            segs[-1][2] += 1
        else:
            segs.append([c, k, 1, vis, s])
    return [tuple(x[:4]) for x in segs]


def test_recorded_root_scripts_in_chunks(exe):
    """The 20 ops_root_* scripts of tests/golden/ops.json: the runs of consecutive local ops cut into
    calls of at most 8, the list ops of a call planned as one chain over the `messages` list as it
    stood before the call."""
    with open(os.path.join(HERE, "golden", "ops.json")) as f:
        cases = [c for c in json.load(f)["cases"] if c["name"].startswith("ops_root_")]
    assert len(cases) == 20
    lines, wants = [], []
    longest = 0
    for c in cases:
        doc = Doc(c["client"])
        steps = c["steps"]
        k = 0
        while k < len(steps):
            if steps[k]["op"] == "apply":
                doc.apply_update(bytes.fromhex(steps[k]["update"]))
                assert doc.encode_state_as_update().hex() == steps[k]["state"]
                k += 1
                continue
            call = []
            while k < len(steps) and steps[k]["op"] != "apply" and len(call) < 8:
                call.append(steps[k])
                k += 1
            segs = _list_segments(doc.encode_state_as_update(), "messages")
            assert sum(n for _, _, n, v in segs if v) == len(json.loads(doc.root_json("messages", "array")))
            ops = []
            for s in call:
                if s["op"] == "array_insert":
                    assert s["root"] == "messages" and s.get("parent_key") is None
                    ops.append((INSERT, s["index"], 0, len(s["anys"])))
                elif s["op"] == "array_delete":
                    ops.append((DELETE, s["index"], s["length"], 0))
            # the list ops through the oracle as one chain, the map ops as they stand (they take clocks)
            want, fields = [], []
            for s in call:
                if s["op"] in ("array_insert", "array_delete"):
                    op = ops[len(want)]
                    clock, effect, failed = _oracle_op(doc, c["client"], "messages", op, [bytes.fromhex(a) for a in s.get("anys", [])])
                    want.append((effect, failed))
                    fields.append(f"{op[0]} {op[1]} {op[2]} {op[3]} {clock}")
                elif s["op"] == "map_set":
                    doc.map_set(s["root"], s["key"], bytes.fromhex(s["any"]))
                else:
                    assert s["op"] == "map_delete", s["op"]
                    doc.map_delete(s["root"], s["key"])
                assert doc.encode_state_as_update().hex() == s["state"]
            if ops:
                longest = max(longest, len(ops))
                lines.append(f"L {c['client']} {len(segs)} " + " ".join(f"{a} {b} {n} {v}" for a, b, n, v in segs) + f" {len(ops)} " + " ".join(fields))
                lines[-1] = " ".join(lines[-1].split())
                wants.append(want)
    out, (f_ranges, f_pieces, f_other) = _run(exe, lines)
    at = flagged = 0
    for want in wants:
        flagged += _check_plans(out[at:at + len(want)], want)
        at += len(want)
    assert at == len(out)
    print(f"{len(lines)} calls with list ops, {at} list ops, longest chain {longest}; flagged: ranges {f_ranges}, pieces {f_pieces}, other {f_other}")
    assert f_other == 0 and f_pieces == 0 and flagged == f_ranges
    # what tests/test_gpu_docs_transact.py's cap of 5 % single ops rests on
    assert f_ranges * 20 <= at, (f_ranges, at)


# ---------------------------------------------------------------- the host analysis
N = -1  # WRITE_NONE
SET, SET_TYPE, MAP_DELETE = 0, 1, 2


def _a(ops):
    return f"A {len(ops)} " + " ".join(f"{op} {root} {pk or '-'} {key or '-'} {ref}" for op, root, pk, key, ref in ops)


ANALYSIS = [
    # the dependent scenarios of tests/test_gpu_docs_write.py
    ("two sets of one key", [(SET, "m", None, "a", 0), (SET, "m", None, "a", 0)], [(N, N, N, 0), (0, N, N, 0)], 2),
    ("a set and a delete of one key", [(SET, "m", None, "live", 0), (MAP_DELETE, "m", None, "live", 0)], [(N, N, N, 0), (0, N, N, 0)], 2),
    ("two ops on one list", [(PUSH, "run", None, None, 0), (DELETE, "run", None, None, 0)], [(N, N, N, 0), (N, 0, N, 0)], 2),
    ("a type and a push into it", [(SET_TYPE, "m", None, "K", 0), (PUSH, "m", "K", None, 0)], [(N, N, N, 0), (N, N, 0, 0)], 1),
    ("a push and the type replaced", [(PUSH, "m", "arr", None, 0), (SET, "m", None, "arr", 0)], [(N, N, N, 0), (N, N, N, 0)], 1),
    ("a failing insert, then a set", [(INSERT, "run", None, None, 0), (SET, "m", None, "a", 0)], [(N, N, N, 0), (N, N, N, 0)], 1),
    ("three sets of distinct keys", [(SET, "m", None, "a", 0), (SET, "m", None, "live", 0), (SET, "m", "sub", "x", 0)], [(N, N, N, 0)] * 3, 1),
    ("a set under a parent and the same key at the root", [(SET, "m", "sub", "x", 0), (SET, "m", None, "x", 0), (SET, "m", "sub", "x", 0)],
     [(N, N, N, 0), (N, N, N, 0), (0, N, N, 0)], 2),
    ("one list name in two roots", [(PUSH, "a", None, None, 0), (PUSH, "b", None, None, 0), (PUSH, "a", "b", None, 0)], [(N, N, N, 0)] * 3, 1),
    # epochs
    ("type, push, type again, push", [(SET_TYPE, "m", None, "K", 0), (PUSH, "m", "K", None, 0), (SET_TYPE, "m", None, "K", 0), (PUSH, "m", "K", None, 0),
                                      (PUSH, "m", "K", None, 0)],
     [(N, N, N, 0), (N, N, 0, 0), (0, N, N, 0), (N, N, 2, 0), (N, 3, 2, 0)], 2),
    ("delete of the parent entry, then an op under it", [(PUSH, "m", "arr", None, 0), (MAP_DELETE, "m", None, "arr", 0), (PUSH, "m", "arr", None, 0),
                                                        (SET, "m", "arr", "k", 0)],
     [(N, N, N, 0), (N, N, N, 0), (N, N, N, WHY_NO_TYPE), (N, N, N, WHY_NO_TYPE)], 1),
    ("a value over the parent entry", [(SET, "m", None, "sub", 0), (SET, "m", "sub", "x", 0)], [(N, N, N, 0), (N, N, N, WHY_NO_TYPE)], 1),
    ("a set of the other kind", [(SET_TYPE, "m", None, "K", 1), (PUSH, "m", "K", None, 0), (SET, "m", "K", "a", 0), (SET, "m", "K", "a", 0),
                                 (SET_TYPE, "m", None, "K", 0), (SET, "m", "K", "a", 0), (DELETE, "m", "K", None, 0)],
     [(N, N, N, 0), (N, N, N, WHY_MISMATCH), (N, N, 0, 0), (2, N, 0, 0), (0, N, N, 0), (N, N, N, WHY_MISMATCH), (N, N, 4, 0)], 2),
    ("a chain of 9", [(PUSH, "l", None, None, 0)] * 9, [(N, N, N, 0)] + [(N, k, N, 0) for k in range(8)], 9),
    ("no op", [], [], 0),
]


def test_host_analysis(exe):
    assert {"two sets of one key", "a set and a delete of one key", "two ops on one list", "a type and a push into it", "a push and the type replaced",
            "a failing insert, then a set"} <= {label for label, _, _, _ in ANALYSIS}
    out, _ = _run(exe, [_a(ops) for _, ops, _, _ in ANALYSIS])
    at = 0
    for label, ops, links, longest in ANALYSIS:
        got = [tuple(int(x) for x in g.split()[1:]) for g in out[at:at + len(ops)]]
        assert got == links, (label, got, links)
        assert out[at + len(ops)] == f"LONGEST {longest}", (label, out[at + len(ops)])
        at += len(ops) + 1
    assert at == len(out)
