"""Local ops for many documents in one device pass (ycrdt_docs_write / crdt_amd.docs_write): YMap.set /
delete and YArray.insert / push / delete encoded over the view of one multi-document merge, one lane
per op (yc_write.hip). Every op's update must equal, byte for byte, the one the single call of its
kind enqueues — Doc.map_set / map_set_type / map_delete / array_insert / array_delete, the host
encoders over the per-document view — its code what that call returns, and, where the fixtures record
it, the document's state must be Yjs 13.5.16's own bytes.

The hand-written updates and their builders are those of tests/test_gpu_docs_json.py.
"""
import json
import os

import pytest

crdt_amd = pytest.importorskip("crdt_amd")

from tests.test_gpu_docs_json import ANY, STRING, TYPE, _alternating_list, any_int, any_str, anys, item, update, vs, vu  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
E_ARG = -6
NOTHING = b"\x00\x00"  # take_local_update with no local op since the last take


def _ops_cases():
    with open(os.path.join(HERE, "golden", "ops.json")) as f:
        return json.load(f)["cases"]


def _step_op(d, s):
    """A recorded step as a docs_write op."""
    op, pk = s["op"], s.get("parent_key")
    if op == "map_set":
        return (op, d, s["root"], (s["key"], bytes.fromhex(s["any"])), pk)
    if op == "map_set_type":
        return (op, d, s["root"], (s["key"], s["type"]), pk)
    if op == "map_delete":
        return (op, d, s["root"], s["key"], pk)
    if op == "array_insert":
        return (op, d, s["root"], (s["index"], [bytes.fromhex(a) for a in s["anys"]]), pk)
    assert op == "array_delete", op
    return (op, d, s["root"], (s["index"], s["length"]), pk)


# ---------------------------------------------------------------- recorded Yjs scripts in lockstep
def test_recorded_scripts_in_lockstep():
    """The 60 recorded scripts as 60 documents: round k issues every script's step k together, the
    `apply` steps through one apply_updates_multi and the local ops through one docs_write."""
    cases = _ops_cases()
    assert len(cases) == 60
    for c in cases:  # what the stats check below relies on
        for s in c["steps"]:
            assert s.get("length", 0) <= 3 and len((s.get("key") or "").encode()) <= 5 and len((s.get("parent_key") or "").encode()) <= 5
    docs = [crdt_amd.Doc(client_id=c["client"]) for c in cases]
    single = issued = rounds_on_device = 0
    touched = set()  # the documents that hold a state: an update was applied (an empty one too) or an op wrote something
    for k in range(max(len(c["steps"]) for c in cases)):
        live = [(d, c["steps"][k]) for d, c in zip(docs, cases) if k < len(c["steps"])]
        applies = [(d, s) for d, s in live if s["op"] == "apply"]
        if applies:
            crdt_amd.apply_updates_multi([d for d, _ in applies], [bytes.fromhex(s["update"]) for _, s in applies])
            touched |= {id(d) for d, _ in applies}
        local = [(d, s) for d, s in live if s["op"] != "apply"]
        if local:
            # where every op must go: a document with something pending takes the single calls, one
            # without state is `empty`, every other one is the device's (no op may be refused there)
            pending = [any(d.pending()) for d, _ in local]
            stateless = [not p and id(d) not in touched for (d, _), p in zip(local, pending)]
            ups, codes, st = crdt_amd.docs_write_stats([_step_op(d, s) for d, s in local])
            print(f"round {k}: {len(local)} ops, {st}")
            assert codes == [0] * len(local), (k, codes)
            touched |= {id(d) for (d, _), u in zip(local, ups) if u}
            assert st["ops_device"] + st["ops_single"] + st["ops_empty"] == len(local) and st["out_bytes"] == sum(map(len, ups)), st
            assert st["ops_single"] == sum(pending) and st["ops_empty"] == sum(stateless), (k, st)
            # (in round 0 every document that writes is still empty: 45 `empty` ops and none for the device)
            assert st["ops_device"] > 0 or k == 0, (k, st)
            rounds_on_device += st["ops_device"] > 0
            single += st["ops_single"]
            issued += sum(pending)
        for d, s in live:
            assert d.encode_state_as_update().hex() == s["state"], (k, s["op"])
    assert single == issued, (single, issued)
    assert rounds_on_device >= 20
    for d, c in zip(docs, cases):
        assert json.loads(d.root_json("users", "map")) == c["json"]["users"], c["name"]
        assert json.loads(d.root_json("messages", "array")) == c["json"]["messages"], c["name"]


# ---------------------------------------------------------------- twin fleets against the single calls
R, Q = 5, 9  # remote clients of the hand-built documents
I1, I2, I3, I4, I5 = (any_int(i) for i in range(1, 6))


def _map_doc(r=R):
    """Root map `m`: a live entry, a deleted one, one whose item holds 2 values, a nested YMap `sub`
    with an entry, a nested YArray `arr` with 2 elements, a deleted nested type and the entry ""."""
    return [update(r, [
        (item(ANY, anys(I1), root="m", psub="live"), 1),          # 0
        (item(ANY, anys(I2), root="m", psub="dead"), 1),          # 1 (deleted)
        (item(ANY, anys(I3, I4), root="m", psub="two"), 2),       # 2-3
        (item(TYPE, vu(1), root="m", psub="sub"), 1),             # 4
        (item(ANY, anys(I5), parent=(r, 4), psub="x"), 1),        # 5
        (item(TYPE, vu(0), root="m", psub="arr"), 1),             # 6
        (item(ANY, anys(I1, I2), parent=(r, 6)), 2),              # 7-8
        (item(TYPE, vu(1), root="m", psub="gone"), 1),            # 9 (deleted)
        (item(ANY, anys(I4), root="m", psub=""), 1),              # 10
        (item(TYPE, vu(0), root="m", psub="earr"), 1),            # 11: an empty nested list
    ], deleted=[(1, 1), (9, 1)])]


def _list_doc():
    """Root lists. `run`: [v v v] D [v]; `dfirst`: D [v v]; `desc`: a run of client Q then one of
    client R; `adj`: two structs of one client adjacent in clock that cannot merge."""
    return [
        update(Q, [(item(ANY, anys(I1, I2), root="desc"), 2)]),
        update(R, [
            (item(ANY, anys(I1, I2, I3), root="run"), 3),         # 0-2
            (item(ANY, anys(I4), origin=(R, 2)), 1),              # 3 (deleted)
            (item(ANY, anys(I5), origin=(R, 3)), 1),              # 4
            (item(ANY, anys(I1), root="dfirst"), 1),              # 5 (deleted)
            (item(ANY, anys(I2, I3), origin=(R, 5)), 2),          # 6-7
            (item(ANY, anys(I3, I4), origin=(Q, 1)), 2),          # 8-9: behind client Q's run in `desc`
            (item(ANY, anys(I1), root="adj"), 1),                 # 10
            (item(STRING, vs("b"), origin=(R, 10)), 1),           # 11
        ], deleted=[(3, 1), (5, 1)]),
    ]


def _own_clock_doc(own, n):
    """The document's own client has written n elements: its next clock is n."""
    return [update(own, [(item(STRING, vs("a" * n), root="s"), n)])] + _map_doc()


LONG_ENTRY = b"b" * 64 + b"L" * 236


def _scenario():
    """(label, own client, updates, [(op, root, arg, parent_key)], path): one document each; `path`
    is where its ops must go when nothing is switched off."""
    V = any_str("v")
    S = []

    def one(label, updates, op, root, arg, pkey=None, path="device", own=None):
        S.append((label, 1000 + len(S) if own is None else own, updates, [(op, root, arg, pkey)], path))

    # ---- map ops
    for key in ("absent", "live", "dead", "two", ""):
        one(f"set {key!r}", _map_doc(), "map_set", "m", (key, V))
        one(f"delete {key!r}", _map_doc(), "map_delete", "m", key)
    one("set type", _map_doc(), "map_set_type", "m", ("fresh", 0))
    one("set type over a value", _map_doc(), "map_set_type", "m", ("live", 1))
    one("set in a root that does not exist", _map_doc(), "map_set", "other", ("k", V))
    one("set under parent", _map_doc(), "map_set", "m", ("x", V), "sub")
    one("set a new key under parent", _map_doc(), "map_set", "m", ("y", V), "sub")
    one("delete under parent", _map_doc(), "map_delete", "m", "x", "sub")
    one("delete absent under parent", _map_doc(), "map_delete", "m", "y", "sub")
    for pk in ("live", "gone", "arr", "nope", "dead"):  # a plain value, a deleted type, a YArray, nothing, a deleted value
        one(f"set under {pk}", _map_doc(), "map_set", "m", ("k", V), pk)
        one(f"delete under {pk}", _map_doc(), "map_delete", "m", "k", pk)
    one("insert under a YMap", _map_doc(), "array_insert", "m", (0, [V]), "sub")
    one("delete under a YMap", _map_doc(), "array_delete", "m", (0, 1), "sub")
    # ---- array insert and push
    one("insert into a root that does not exist", _list_doc(), "array_insert", "fresh", (0, [V, I1]))
    one("push into a root that does not exist", _list_doc(), "array_push", "fresh", [V])
    one("insert into an empty nested list", _map_doc(), "array_insert", "m", (0, [V]), "earr")
    one("insert at 0 before a deleted first segment", _list_doc(), "array_insert", "dfirst", (0, [V]))
    one("insert at 0", _list_doc(), "array_insert", "run", (0, [V]))
    one("insert in the middle of a run", _list_doc(), "array_insert", "run", (2, [V, V]))
    one("insert at the end of a run a deleted segment follows", _list_doc(), "array_insert", "run", (3, [V]))
    one("insert at the end of the list", _list_doc(), "array_insert", "run", (4, [V]))
    one("push", _list_doc(), "array_push", "run", [V, I2, I3])
    one("insert at length + 1", _list_doc(), "array_insert", "run", (5, [V]))
    one("insert nothing", _list_doc(), "array_insert", "run", (1, []))
    one("insert nothing past the end", _list_doc(), "array_insert", "run", (9, []))
    one("push nothing", _list_doc(), "array_push", "run", [])
    one("insert into a nested list", _map_doc(), "array_insert", "m", (1, [V]), "arr")
    one("push onto a nested list", _map_doc(), "array_push", "m", [V], "arr")
    one("insert between two clients' runs", _list_doc(), "array_insert", "desc", (2, [V]))
    # ---- array delete
    one("delete inside one run", _list_doc(), "array_delete", "run", (1, 1))
    one("delete a whole run and more", _list_doc(), "array_delete", "run", (0, 4))
    one("delete across runs of descending clients", _list_doc(), "array_delete", "desc", (1, 2))
    one("delete across runs adjacent in clock", _list_doc(), "array_delete", "adj", (0, 2))
    one("delete across a deleted segment", _list_doc(), "array_delete", "run", (2, 2))
    one("delete past the end", _list_doc(), "array_delete", "run", (3, 5))
    one("delete wholly past the end", _list_doc(), "array_delete", "run", (10, 2))
    one("delete nothing", _list_doc(), "array_delete", "run", (1, 0))
    one("delete from a root that does not exist", _list_doc(), "array_delete", "fresh", (0, 1))
    one("delete in a nested list", _map_doc(), "array_delete", "m", (0, 2), "arr")
    one("delete across 8 segments", [_alternating_list(9, root="alt")], "array_delete", "alt", (0, 8))
    one("delete across 8 segments from 1", [_alternating_list(9, root="alt")], "array_delete", "alt", (1, 8))
    one("delete across 9 segments", [_alternating_list(9, root="alt")], "array_delete", "alt", (0, 9), path="single")
    one("delete across 9 segments and past the end", [_alternating_list(9, root="alt")], "array_delete", "alt", (0, 12), path="single")
    # ---- ids
    one("own client 0xFFFFFFFF", _map_doc(), "map_set", "m", ("live", V), own=0xFFFFFFFF)
    one("own client 0", _map_doc(), "array_push", "m", [V], "arr", own=0)
    one("origin of client 0xFFFFFFFF", _map_doc(0xFFFFFFFF), "map_set", "m", ("two", V))
    one("parent of client 0xFFFFFFFF", _map_doc(0xFFFFFFFF), "map_set", "m", ("z", V), "sub")
    one("range of client 0xFFFFFFFF", _map_doc(0xFFFFFFFF), "map_delete", "m", "two")
    for n in (127, 128, 16384):
        one(f"own next clock {n}", _own_clock_doc(70000 + n, n), "map_set", "m", ("live", V), own=70000 + n)
        one(f"origin clock {n - 1}", _own_clock_doc(80000 + n, n), "array_push", "s", [V], own=3)
    # ---- names
    name_doc = [update(R, [(item(ANY, anys(I1), root="m", psub="k" * 64), 1), (item(TYPE, vu(1), root="m", psub="p" * 64), 1)])]
    one("a key of 64 bytes", name_doc, "map_set", "m", ("k" * 64, V))
    one("a new key of 64 bytes", name_doc, "map_set", "m", ("j" * 64, V))
    one("a parent key of 64 bytes", name_doc, "map_set", "m", ("a", V), "p" * 64)
    name_doc = [update(R, [(item(ANY, anys(I1), root="m", psub="k" * 65), 1), (item(TYPE, vu(1), root="m", psub="p" * 65), 1)])]
    one("a key of 65 bytes", name_doc, "map_set", "m", ("k" * 65, V), path="single")
    one("a parent key of 65 bytes", name_doc, "map_set", "m", ("a", V), "p" * 65, path="single")
    long_doc = [update(R, [(item(ANY, anys(I1), root="m", psub=b"b" * 64), 1), (item(ANY, anys(I2), root="m", psub=LONG_ENTRY), 1)])]
    one("a long entry beside the request's prefix", long_doc, "map_set", "m", ("b" * 64, V), path="single")
    one("a long entry elsewhere", long_doc, "map_set", "m", ("b" * 63 + "a", V))
    # ---- values
    one("a bad any value", _map_doc(), "map_set", "m", ("live", b"\xff"))
    one("a bad any value in a list", _list_doc(), "array_push", "run", [V, b"\x7d"])
    # ---- several ops per document
    S.append(("three sets of distinct keys", 2001, _map_doc(), [("map_set", "m", ("a", V), None), ("map_set", "m", ("live", V), None),
                                                               ("map_set", "m", ("x", V), "sub")], "device"))
    S.append(("items of several lengths", 2002, _list_doc(), [("map_set", "m", ("a", V), None), ("array_push", "run", [V, V, V], None),
                                                              ("array_delete", "desc", (0, 3), None), ("array_insert", "adj", (1, [V]), None),
                                                              ("map_set_type", "m", ("t", 1), None)], "device"))
    S.append(("a bad value between two sets", 2003, _map_doc(), [("map_set", "m", ("a", V), None), ("map_set", "m", ("b", b"\xff"), None),
                                                                ("map_set", "m", ("c", V), None)], "device"))
    S.append(("a failing op last", 2004, _list_doc(), [("map_set", "m", ("a", V), None), ("array_insert", "run", (9, [V]), None)], "device"))
    S.append(("two sets of one key", 2005, _map_doc(), [("map_set", "m", ("a", V), None), ("map_set", "m", ("a", I1), None)], "single"))
    S.append(("a set and a delete of one key", 2006, _map_doc(), [("map_set", "m", ("live", V), None), ("map_delete", "m", "live", None)], "single"))
    S.append(("two ops on one list", 2007, _list_doc(), [("array_push", "run", [V], None), ("array_delete", "run", (0, 1), None)], "single"))
    S.append(("a type and a push into it", 2008, _map_doc(), [("map_set_type", "m", ("K", 0), None), ("array_push", "m", [V], "K")], "single"))
    S.append(("a push and the type replaced", 2009, _map_doc(), [("array_push", "m", [V], "arr"), ("map_set", "m", ("arr", V), None)], "single"))
    S.append(("a failing insert, then a set", 2010, _list_doc(), [("array_insert", "run", (9, [V]), None), ("map_set", "m", ("a", V), None)], "single"))
    # ---- an empty document, and one with pending structs
    S.append(("an empty document", 2011, [], [("map_set", "m", ("a", V), None), ("array_push", "l", [V], None), ("map_delete", "m", "a", None)], "empty"))
    with open(os.path.join(HERE, "golden", "pending.json")) as f:
        gap = next(c for c in json.load(f)["cases"] if c["name"] == "kat_gap")
    S.append(("pending structs", 2012, [bytes.fromhex(gap["updates"][0])], [("map_set", "m", ("a", V), None)], "single"))
    return S


def _doc(client, updates, engine):
    d = crdt_amd.Doc(client_id=client, engine=engine)
    if updates:
        d.apply_updates(list(updates))
        d.flush()
    d.track_local(True)
    return d


def _single(d, op, root, arg, pkey):
    """The op through Doc's single calls: the code, and the update it enqueued (b"" where none)."""
    try:
        if op == "map_set":
            d.map_set(root, arg[0], arg[1], parent_key=pkey)
        elif op == "map_set_type":
            d.map_set_type(root, arg[0], arg[1], parent_key=pkey)
        elif op == "map_delete":
            d.map_delete(root, arg, parent_key=pkey)
        elif op == "array_insert":
            d.array_insert(root, arg[0], arg[1], parent_key=pkey)
        elif op == "array_push":
            d.array_insert(root, d.array_length(root, parent_key=pkey), arg, parent_key=pkey)
        else:
            d.array_delete(root, arg[0], arg[1], parent_key=pkey)
        code = 0
    except crdt_amd.YcrdtError as e:
        assert e.kind == "ARG", (op, root, arg, pkey, e)
        code = e.code
    u = d.take_local_update()
    return code, b"" if u == NOTHING else u


def _twins(scenario, engine=None, mode="default"):
    """Fleet A through one docs_write call, fleet B through the single calls: every update, code and
    final state compared. Returns A's updates and the stats."""
    A = [_doc(own, ups, engine) for _, own, ups, _, _ in scenario]
    B = [_doc(own, ups, engine) for _, own, ups, _, _ in scenario]
    call = [(op, a, root, arg, pkey) for a, (_, _, _, ops, _) in zip(A, scenario) for op, root, arg, pkey in ops]
    ups, codes, st = crdt_amd.docs_write_stats(call, engine=engine)
    print(mode, st)
    assert len(ups) == len(codes) == len(call)
    assert st["ops_device"] + st["ops_single"] + st["ops_empty"] == len(call), st
    assert st["out_bytes"] == sum(map(len, ups)) and st["ranges_max"] == 8 and st["name_max"] == 64, st
    i = 0
    noop = 0
    for a, b, (label, _, _, ops, _) in zip(A, B, scenario):
        mine = []
        for op, root, arg, pkey in ops:
            code, want = _single(b, op, root, arg, pkey)
            print(f"  {label}: {op} code {codes[i]} / {code}, {ups[i].hex()} / {want.hex()}")
            assert codes[i] == code, (label, op, codes[i], code)
            assert ups[i] == want, (label, op, ups[i].hex(), want.hex())
            noop += not want and not code
            if ups[i]:
                mine.append(ups[i])
            i += 1
        # the updates were enqueued as local transactions, and both fleets hold the same documents
        took = a.take_local_update()
        assert took == (NOTHING if not mine else mine[0] if len(mine) == 1 else crdt_amd.merge_updates(mine, engine=engine)), label
        assert a.encode_state_as_update() == b.encode_state_as_update(), label
        assert a.encode_state_vector() == b.encode_state_vector(), label
        roots = {root for _, root, _, _ in ops} | {"m"}
        for root in roots:
            for kind in ("map", "array"):
                assert a.root_json(root, kind) == b.root_json(root, kind), (label, root)
    assert st["ops_noop"] == noop, (st, noop)
    return ups, codes, st


def _paths(scenario):
    n = {"device": 0, "single": 0, "empty": 0}
    for _, _, _, ops, path in scenario:
        n[path] += len(ops)
    return n


@pytest.fixture(scope="module")
def scenario():
    return _scenario()


@pytest.fixture(scope="module")
def default_run(scenario):
    return _twins(scenario)


def test_twin_fleets(scenario, default_run):
    ups, codes, st = default_run
    want = _paths(scenario)
    assert (st["ops_device"], st["ops_single"], st["ops_empty"]) == (want["device"], want["single"], want["empty"]), (st, want)
    by_label, own_of = {}, {}
    i = 0
    for label, own, _, ops, _ in scenario:
        assert label not in by_label
        by_label[label] = (ups[i:i + len(ops)], codes[i:i + len(ops)])
        own_of[label] = own
        i += len(ops)
    # what the cases are there for, spelled out on a few of them (the bytes are the single calls' above)
    for pk in ("live", "gone", "arr", "nope", "dead"):
        assert by_label[f"set under {pk}"] == ([b""], [E_ARG]) and by_label[f"delete under {pk}"] == ([b""], [E_ARG])
    for label in ("delete 'absent'", "delete 'dead'", "insert nothing", "push nothing", "delete nothing", "delete absent under parent"):
        assert by_label[label] == ([b""], [0]), label
    for label in ("insert at length + 1", "insert nothing past the end", "delete wholly past the end", "a bad any value",
                  "delete from a root that does not exist"):
        assert by_label[label] == ([b""], [E_ARG]), label
    u, c = by_label["delete past the end"]
    assert c == [E_ARG] and u == [bytes([0, 1, R, 1, 4, 1])]
    assert by_label["delete across runs adjacent in clock"][0] == [bytes([0, 1, R, 1, 10, 2])]  # merged
    assert by_label["delete across a deleted segment"][0] == [bytes([0, 1, R, 2, 2, 1, 4, 1])]
    assert by_label["delete across runs of descending clients"][0] == [bytes([0, 2, R, 1, 8, 1, Q, 1, 1, 1])]
    assert by_label["delete 'two'"][0] == [bytes([0, 1, R, 1, 2, 2])]
    V = any_str("v")
    head = {label: bytes([1, 1]) + vu(own) for label, own in own_of.items()}  # one client, one struct, the client (2 bytes here)
    assert by_label["set 'two'"][0] == [head["set 'two'"] + bytes([0, 0xA8, R, 3]) + anys(V) + b"\x00"]  # origin: the item's last clock
    assert by_label["set 'dead'"][0] == [head["set 'dead'"] + bytes([0, 0xA8, R, 1]) + anys(V) + b"\x00"]  # origin: the deleted item
    assert by_label["insert at 0 before a deleted first segment"][0][0][5:8] == bytes([0x48, R, 5])  # right origin: the deleted segment
    assert by_label["insert at the end of a run a deleted segment follows"][0][0][5:10] == bytes([0xC8, R, 2, R, 3])
    three = by_label["three sets of distinct keys"][0]
    assert [u[:5] for u in three] == [head["three sets of distinct keys"] + bytes([k]) for k in range(3)]  # consecutive clocks
    several = by_label["items of several lengths"][0]
    assert [u[4] for u in (several[0], several[1], several[3], several[4])] == [0, 1, 4, 5]  # clocks: 1, 3, (a delete), 1, 1
    assert by_label["own next clock 16384"][0][0][:8] == bytes([1, 1]) + vu(70000 + 16384) + vu(16384)


def test_twin_fleets_in_three_passes(monkeypatch, scenario, default_run):
    sizes = [len(_doc(1, ups, None).encode_state_as_update()) for _, _, ups, _, path in scenario if path == "device"]
    padded = sum((s + 63) // 64 * 64 for s in sizes)
    monkeypatch.setenv("YCRDT_DOCS_WRITE_PASS_BYTES", str(padded * 2 // 5))
    ups, codes, st = _twins(scenario, mode="three passes")
    assert (ups, codes) == default_run[:2]
    # (two passes of 2/5 of the device documents' padded bytes cannot hold them: there are at least three)
    assert (st["ops_device"], st["ops_single"], st["ops_empty"]) == tuple(default_run[2][k] for k in ("ops_device", "ops_single", "ops_empty"))


def test_twin_fleets_switched_off(monkeypatch, scenario, default_run):
    monkeypatch.setenv("YCRDT_DOCS_WRITE", "0")
    ups, codes, st = _twins(scenario, mode="switched off")
    assert (ups, codes) == default_run[:2]
    assert st["ops_device"] == 0 and st["ops_single"] == len(ups), st


def test_twin_fleets_compat_135(scenario, default_run):
    e135 = crdt_amd.Engine(compat=135)
    ups, codes, st = _twins(scenario, engine=e135, mode="compat 135")
    assert (ups, codes) == default_run[:2]
    assert st["ops_device"] == 0 and st["ops_empty"] == 0 and st["ops_single"] == len(ups), st  # (the empty document's ops too)


def test_no_op_and_argument_errors():
    import ctypes

    ups, codes, st = crdt_amd.docs_write_stats([])
    assert ups == [] and codes == [] and st["out_bytes"] == 0 and st["ops_device"] == st["ops_single"] == st["ops_empty"] == 0
    d = _doc(7, _map_doc(), None)
    before = d.encode_state_as_update()
    with pytest.raises(crdt_amd.YcrdtError):
        crdt_amd.docs_write([("map_set", d, "m", ("a", I1))], engine=crdt_amd.Engine())  # a document of another engine
    with pytest.raises(ValueError):
        crdt_amd.docs_write([("map_has", d, "m", "a")])
    L = crdt_amd.lib()
    h = d._h.value
    for doc, root, op in ((None, b"m", 0), (h, None, 0), (h, b"m", 6), (h, b"m", -1)):
        wr = (crdt_amd._Write * 2)()
        wr[0].doc, wr[0].root, wr[0].key, wr[0].any, wr[0].any_len, wr[0].op = h, b"m", b"first", I1, 2, 0  # a good op in front: nothing of it is enqueued
        wr[1].doc, wr[1].root, wr[1].key, wr[1].op = doc, root, b"a", op
        out, offs, codes = crdt_amd._Out(), (ctypes.c_uint64 * 3)(), (ctypes.c_int32 * 2)()
        assert L.ycrdt_docs_write(d.engine._h, wr, 2, ctypes.byref(out), offs, codes, None) == E_ARG
        assert not out.ptr and out.len == 0
    assert d.encode_state_as_update() == before and d.take_local_update() == NOTHING
    # a null key is the op's own failure, as in the single call
    wr = (crdt_amd._Write * 1)()
    wr[0].doc, wr[0].root, wr[0].op = h, b"m", 2
    out, offs, codes = crdt_amd._Out(), (ctypes.c_uint64 * 2)(), (ctypes.c_int32 * 1)()
    assert L.ycrdt_docs_write(d.engine._h, wr, 1, ctypes.byref(out), offs, codes, None) == 0
    assert codes[0] == E_ARG and offs[1] == 0 and b"null arg" in L.ycrdt_last_error()
    L.ycrdt_free(ctypes.byref(out))


# ---------------------------------------------------------------- write, then read
def test_write_then_read_and_diff():
    n = 200
    pre = [update(R, [(item(ANY, anys(any_int(i % 60)), root="users", psub="k"), 1), (item(ANY, anys(I1, I2), root="log"), 2)]) for i in range(n)]
    docs = [_doc(3000 + i, [pre[i]], None) for i in range(n)]
    svs = [d.encode_state_vector() for d in docs]
    ops = []
    for i, d in enumerate(docs):
        ops.append(("map_set", d, "users", ("k" if i % 2 else f"n{i}", any_str(f"value {i}"))))
        ops.append(("array_push", d, "log", [any_int(i % 60), any_str("x")]))
    ups, codes, st = crdt_amd.docs_write_stats(ops)
    assert codes == [0] * len(ops) and st["ops_device"] == len(ops), st
    reads = []
    for i, d in enumerate(docs):
        reads += [("map_get", d, "users", "k" if i % 2 else f"n{i}"), ("array_get", d, "log", 2), ("array_get", d, "log", 3), ("array_length", d, "log")]
    got, rst = crdt_amd.docs_read_stats(reads)
    assert rst["reads_single"] == 0, rst
    for i in range(n):
        assert got[4 * i:4 * i + 4] == [(1, json.dumps(f"value {i}")), (1, str(i % 60)), (1, '"x"'), 4], i
    # The sync reply against the pre-write state vectors is the document's two updates merged. Where
    # the ops overwrite nothing (the even documents: a new key) that is merge_updates of the returned
    # updates, byte for byte. A set of an existing key differs from it in two ways that are Yjs's
    # own: integrating the new item deletes the one it overwrites, so the document's reply carries
    # that delete set and the op's update cannot; and an update read without a document
    # (Y.mergeUpdates) cannot know the parentSub of an item that names its origin and clears bit 6 of
    # its info byte, where a document's encode sets it. So for every document a peer that holds the
    # pre-write state and receives the returned updates must give the same reply.
    diffs = crdt_amd.docs_diff(docs, svs)
    for i in range(0, n, 2):
        assert diffs[i] == crdt_amd.merge_updates(ups[2 * i:2 * i + 2]), i
    merged = crdt_amd.merge_updates(ups[2:4])
    assert diffs[1][:5] == merged[:5] and diffs[1][5] == merged[5] | 0x20 and diffs[1][6:len(merged) - 1] == merged[6:-1]
    assert diffs[1][len(merged) - 1:] == bytes([1, R, 1, 0, 1])  # the overwritten item of client R
    peers = [crdt_amd.Doc(client_id=9000 + i) for i in range(n)]
    crdt_amd.apply_updates_multi([p for p in peers for _ in range(3)], [u for i in range(n) for u in (pre[i], ups[2 * i], ups[2 * i + 1])])
    assert crdt_amd.docs_diff(peers, svs) == diffs
