"""A document's dependent ops planned in one device pass (ycrdt_docs_transact / crdt_amd.docs_transact;
DESIGN.md §5.2h): two ops of one map entry or one list, and a map_set_type followed by ops under its
key, no longer send their document to the single calls. Op i's update must equal, byte for byte, the
one the single call of its kind enqueues once the call's earlier ops on that document have run —
Doc.map_set / map_set_type / map_delete / array_insert / array_delete in order on a twin document —
and its code what that call returns.

The hand-built documents, the twin-fleet helpers and the independent scenarios are those of
tests/test_gpu_docs_write.py."""
import json

import pytest

crdt_amd = pytest.importorskip("crdt_amd")

from tests.test_gpu_docs_json import ANY, TYPE, _alternating_list, any_str, anys, item, update, vu  # noqa: E402
from tests.test_gpu_docs_write import (E_ARG, I1, I2, I3, NOTHING, R, _doc, _list_doc, _map_doc, _ops_cases, _scenario, _single,  # noqa: E402
                                       _step_op)

pytestmark = pytest.mark.gpu

V = any_str("v")
P64 = "p" * 64


def _nested_doc():
    """Root map `m` with a YArray of two elements under a 64-byte key."""
    return [update(R, [(item(TYPE, vu(0), root="m", psub=P64), 1), (item(ANY, anys(I1, I2), parent=(R, 0)), 2)])]


def _dependent():
    """(label, own client, updates, [(op, root, arg, parent_key)], (ops_device, ops_single, ops_empty, ops_chained))"""
    S = []

    def add(label, updates, ops, want):
        S.append((label, 4000 + len(S), updates, ops, want))

    def sets(*kv):
        return [("map_set", "m", (k, v), None) for k, v in kv]

    add("two sets of one key", _map_doc(), sets(("a", V), ("a", I1)), (2, 0, 0, 1))
    add("set then delete", _map_doc(), sets(("live", V)) + [("map_delete", "m", "live", None)], (2, 0, 0, 1))
    add("delete then set", _map_doc(), [("map_delete", "m", "live", None)] + sets(("live", V)), (2, 0, 0, 1))
    add("delete twice", _map_doc(), [("map_delete", "m", "two", None), ("map_delete", "m", "two", None)], (2, 0, 0, 1))
    add("set, delete, delete, set, delete", _map_doc(), sets(("n", V)) + [("map_delete", "m", "n", None)] * 2 + sets(("n", I1)) + [("map_delete", "m", "n", None)],
        (5, 0, 0, 4))
    add("set of a dead entry twice", _map_doc(), sets(("dead", V), ("dead", I1)), (2, 0, 0, 1))
    add("a type and a push into it", _map_doc(), [("map_set_type", "m", ("K", 0), None), ("array_push", "m", [V], "K")], (2, 0, 0, 1))
    add("a map type and a set in it", _map_doc(), [("map_set_type", "m", ("K", 1), None), ("map_set", "m", ("a", V), "K"), ("map_delete", "m", "b", "K")], (3, 0, 0, 2))
    add("a type over a live type", _map_doc(), [("map_set_type", "m", ("arr", 0), None), ("array_push", "m", [V], "arr"), ("array_insert", "m", (0, [I1]), "arr")],
        (3, 0, 0, 2))
    add("type, push, push, delete in the new list", _map_doc(),
        [("map_set_type", "m", ("K", 0), None), ("array_push", "m", [V, I1], "K"), ("array_push", "m", [I2], "K"), ("array_delete", "m", (1, 2), "K")], (4, 0, 0, 3))
    add("type, push, type again, push", _map_doc(),
        [("map_set_type", "m", ("K", 0), None), ("array_push", "m", [V], "K"), ("map_set_type", "m", ("K", 0), None), ("array_push", "m", [I1], "K")], (4, 0, 0, 3))
    add("a type replaced by a value, then an op under it", _map_doc(),
        [("map_set_type", "m", ("K", 0), None), ("array_push", "m", [V], "K"), ("map_set", "m", ("K", V), None), ("array_push", "m", [V], "K")], (4, 0, 0, 3))
    add("a type of the other kind, then an op under it", _map_doc(), [("map_set_type", "m", ("arr", 1), None), ("array_push", "m", [V], "arr")], (2, 0, 0, 1))
    add("the parent entry deleted, then an op under it", _map_doc(), [("map_delete", "m", "sub", None), ("map_set", "m", ("x", V), "sub")], (2, 0, 0, 1))
    add("push then delete of the pushed element", _list_doc(), [("array_push", "run", [V], None), ("array_delete", "run", (4, 1), None)], (2, 0, 0, 1))
    add("insert inside an earlier run", _list_doc(), [("array_insert", "run", (1, [V, I1, I2]), None), ("array_insert", "run", (2, [V]), None)], (2, 0, 0, 1))
    add("insert at 0 three times", _list_doc(), [("array_insert", "dfirst", (0, [V]), None)] * 3, (3, 0, 0, 2))
    add("insert behind a view element a deleted segment follows, twice", _list_doc(), [("array_insert", "run", (3, [V]), None)] * 2, (2, 0, 0, 1))
    add("insert behind the run that stands before a deleted segment", _list_doc(), [("array_insert", "run", (3, [V, I1]), None), ("array_insert", "run", (5, [I2]), None)],
        (2, 0, 0, 1))
    add("delete across a view piece, a run and a view piece", _list_doc(), [("array_insert", "run", (2, [V, I1]), None), ("array_delete", "run", (1, 4), None)],
        (2, 0, 0, 1))
    add("a delete past the end last", _list_doc(), [("array_push", "run", [V], None), ("array_delete", "run", (3, 9), None)], (2, 0, 0, 1))
    add("a chain of 8", _list_doc(), [("array_push", "run", [V], None)] * 8, (8, 0, 0, 7))
    add("a chain of 9", _list_doc(), [("array_push", "run", [V], None)] * 9, (0, 9, 0, 0))
    add("8 sets of one key", _map_doc(), sets(*[("a", V)] * 8), (8, 0, 0, 7))
    add("9 sets of one key", _map_doc(), sets(*[("a", V)] * 9), (0, 9, 0, 0))
    add("a failing op in the middle", _list_doc(), [("array_push", "run", [V], None), ("array_insert", "run", (99, [V]), None), ("array_push", "run", [V], None)],
        (0, 3, 0, 0))
    add("a failing op last", _list_doc(), [("array_push", "run", [V], None), ("array_insert", "run", (99, [V]), None)], (2, 0, 0, 1))
    add("a nested list under a 64-byte parent key", _nested_doc(),
        [("array_push", "m", [V], P64), ("array_insert", "m", (1, [I3]), P64), ("array_delete", "m", (0, 2), P64)], (3, 0, 0, 2))
    add("an 8-range delete", [_alternating_list(9, root="alt")], [("array_push", "alt", [V], None), ("array_delete", "alt", (3, 8), None)], (2, 0, 0, 1))
    add("a 9-range delete", [_alternating_list(9, root="alt")], [("array_push", "alt", [V], None), ("array_delete", "alt", (0, 9), None)], (0, 2, 0, 0))
    add("an empty document", [], sets(("a", V), ("a", I1)), (0, 0, 2, 0))
    return S


def _twins(scenario, engine=None, together=False):
    """Fleet A through docs_transact — one call per scenario, or one over all of them —, fleet B through
    the single calls in order: every update, code and final state compared. Returns A's updates, codes
    and the stats of every call."""
    A = [_doc(own, ups, engine) for _, own, ups, _, _ in scenario]
    B = [_doc(own, ups, engine) for _, own, ups, _, _ in scenario]
    calls = [[(op, a, root, arg, pkey) for op, root, arg, pkey in ops] for a, (_, _, _, ops, _) in zip(A, scenario)]
    if together:
        calls = [[op for call in calls for op in call]]
    ups, codes, stats = [], [], []
    for call in calls:
        u, c, st = crdt_amd.docs_transact_stats(call, engine=engine)
        assert len(u) == len(c) == len(call)
        assert st["ops_device"] + st["ops_single"] + st["ops_empty"] == len(call) and st["ops_chained"] <= st["ops_device"], st
        assert st["out_bytes"] == sum(map(len, u)) and (st["ranges_max"], st["name_max"], st["chain_max"]) == (8, 64, 8), st
        ups += u
        codes += c
        stats.append(st)
    i = 0
    for a, b, (label, _, _, ops, _) in zip(A, B, scenario):
        mine = []
        for op, root, arg, pkey in ops:
            code, want = _single(b, op, root, arg, pkey)
            print(f"  {label}: {op} code {codes[i]} / {code}, {ups[i].hex()} / {want.hex()}")
            assert codes[i] == code, (label, op, codes[i], code)
            assert ups[i] == want, (label, op, ups[i].hex(), want.hex())
            if ups[i]:
                mine.append(ups[i])
            i += 1
        took = a.take_local_update()
        assert took == (NOTHING if not mine else mine[0] if len(mine) == 1 else crdt_amd.merge_updates(mine, engine=engine)), label
        assert a.encode_state_as_update() == b.encode_state_as_update(), label
        assert a.encode_state_vector() == b.encode_state_vector(), label
        for root in {root for _, root, _, _ in ops} | {"m"}:
            for kind in ("map", "array"):
                assert a.root_json(root, kind) == b.root_json(root, kind), (label, root)
    return ups, codes, stats


@pytest.fixture(scope="module")
def dependent():
    return _dependent()


@pytest.fixture(scope="module")
def dependent_run(dependent):
    return _twins(dependent)


def _stats(st):
    return (st["ops_device"], st["ops_single"], st["ops_empty"], st["ops_chained"])


def test_dependent_scenarios(dependent, dependent_run):
    ups, codes, stats = dependent_run
    by_label, own_of = {}, {}
    i = 0
    for (label, own, _, ops, want), st in zip(dependent, stats):
        own_of[label] = vu(own)
        print(label, st)
        assert _stats(st) == want, (label, st, want)
        by_label[label] = (ups[i:i + len(ops)], codes[i:i + len(ops)])
        i += len(ops)
    # what the cases are there for, spelled out on a few of them (the bytes are the single calls' above)
    u, c = by_label["delete twice"]
    assert c == [0, 0] and u == [bytes([0, 1, R, 1, 2, 2]), b""]
    u, c = by_label["set, delete, delete, set, delete"]
    own = own_of["set, delete, delete, set, delete"]
    assert c == [0] * 5 and u[1] == bytes([0, 1]) + own + bytes([1, 0, 1]) and u[2] == b"" and u[4] == bytes([0, 1]) + own + bytes([1, 1, 1])
    assert u[3].startswith(bytes([1, 1]) + own + bytes([1, 0xA8]) + own + bytes([0]))  # origin: the deleted first set
    for label in ("a type replaced by a value, then an op under it", "a type of the other kind, then an op under it", "the parent entry deleted, then an op under it",
                  "a failing op last"):
        u, c = by_label[label]
        assert c[-1] == E_ARG and u[-1] == b"" and c[:-1] == [0] * (len(c) - 1), label
    u, c = by_label["a delete past the end last"]
    assert c == [0, E_ARG] and u[1] != b""
    u, _ = by_label["a type and a push into it"]
    own = own_of["a type and a push into it"]
    assert u[1].startswith(bytes([1, 1]) + own + bytes([1, 0x08, 0]) + own + bytes([0]))  # parent: the type item of this call
    u, _ = by_label["insert behind a view element a deleted segment follows, twice"]
    own = own_of["insert behind a view element a deleted segment follows, twice"]
    assert u[0].startswith(bytes([1, 1]) + own + bytes([0, 0xC8, R, 2, R, 3]))  # right origin: the deleted segment
    assert u[1].startswith(bytes([1, 1]) + own + bytes([1, 0xC8, R, 2]) + own + bytes([0]))  # ... then the first run


def test_dependent_scenarios_in_one_call(dependent, dependent_run):
    ups, codes, stats = _twins(dependent, together=True)
    assert (ups, codes) == dependent_run[:2]
    assert _stats(stats[0]) == tuple(sum(w[k] for *_, w in dependent) for k in range(4))


def test_dependent_scenarios_switched_off(monkeypatch, dependent, dependent_run):
    monkeypatch.setenv("YCRDT_DOCS_TRANSACT", "0")
    ups, codes, stats = _twins(dependent, together=True)
    assert (ups, codes) == dependent_run[:2]
    assert _stats(stats[0]) == (0, len(ups), 0, 0), stats


def test_six_documents_in_three_passes(monkeypatch, dependent, dependent_run):
    six = [s for s in dependent if s[4][0] and s[0] != "a chain of 8"][:6]
    assert len(six) == 6
    whole = _twins(six, together=True)
    sizes = [len(_doc(1, ups, None).encode_state_as_update()) for _, _, ups, _, _ in six]
    padded = sum((s + 63) // 64 * 64 for s in sizes)
    # (two passes of 2/5 of the padded bytes cannot hold the documents: there are at least three)
    monkeypatch.setenv("YCRDT_DOCS_TRANSACT_PASS_BYTES", str(padded * 2 // 5))
    ups, codes, stats = _twins(six, together=True)
    assert (ups, codes) == whole[:2] and _stats(stats[0]) == _stats(whole[2][0])
    assert _stats(stats[0]) == tuple(sum(w[k] for *_, w in six) for k in range(4))


# ---------------------------------------------------------------- the independent scenarios of docs_write
NOW_DEVICE = {"two sets of one key": 1, "a set and a delete of one key": 1, "two ops on one list": 1, "a type and a push into it": 1,
              "a push and the type replaced": 0}  # label: its chained ops ("a failing insert, then a set" stays single: the failed op is not the last)


def test_independent_scenarios():
    """tests/test_gpu_docs_write.py's scenarios through docs_transact: docs_write's bytes and codes, and
    its paths but for the dependent documents that now stay on the device. (They share the call's one
    pass, so k_tplan plans every op here, the ones without a link too.)"""
    scenario = _scenario()
    A = [_doc(own, ups, None) for _, own, ups, _, _ in scenario]
    C = [_doc(own, ups, None) for _, own, ups, _, _ in scenario]
    mk = lambda docs: [(op, d, root, arg, pkey) for d, (_, _, _, ops, _) in zip(docs, scenario) for op, root, arg, pkey in ops]  # noqa: E731
    ups, codes, st = crdt_amd.docs_transact_stats(mk(A))
    wups, wcodes, wst = crdt_amd.docs_write_stats(mk(C))
    print(st, wst)
    assert (ups, codes) == (wups, wcodes)
    want = {"device": 0, "single": 0, "empty": 0}
    for label, _, _, ops, path in scenario:
        want["device" if label in NOW_DEVICE else path] += len(ops)
    assert set(NOW_DEVICE) <= {s[0] for s in scenario}
    assert _stats(st) == (want["device"], want["single"], want["empty"], sum(NOW_DEVICE.values())), (st, want)
    assert st["ops_noop"] == wst["ops_noop"] and st["out_bytes"] == wst["out_bytes"]
    moved = sum(len(ops) for label, _, _, ops, _ in scenario if label in NOW_DEVICE)
    assert (wst["ops_device"], wst["ops_single"]) == (st["ops_device"] - moved, st["ops_single"] + moved)
    for a, c, (label, _, _, ops, _) in zip(A, C, scenario):
        assert a.take_local_update() == c.take_local_update(), label
        assert a.encode_state_as_update() == c.encode_state_as_update(), label


def test_no_op_and_argument_errors():
    import ctypes

    ups, codes, st = crdt_amd.docs_transact_stats([])
    assert ups == [] and codes == [] and st["out_bytes"] == 0 and _stats(st) == (0, 0, 0, 0) and st["chain_max"] == 8
    d = _doc(7, _map_doc(), None)
    before = d.encode_state_as_update()
    with pytest.raises(crdt_amd.YcrdtError):
        crdt_amd.docs_transact([("map_set", d, "m", ("a", I1))], engine=crdt_amd.Engine())  # a document of another engine
    L = crdt_amd.lib()
    h = d._h.value
    for doc, root, op in ((None, b"m", 0), (h, None, 0), (h, b"m", 6), (h, b"m", -1)):
        wr = (crdt_amd._Write * 2)()
        wr[0].doc, wr[0].root, wr[0].key, wr[0].any, wr[0].any_len, wr[0].op = h, b"m", b"first", I1, 2, 0  # a good op in front: nothing of it is enqueued
        wr[1].doc, wr[1].root, wr[1].key, wr[1].op = doc, root, b"a", op
        out, offs, codes = crdt_amd._Out(), (ctypes.c_uint64 * 3)(), (ctypes.c_int32 * 2)()
        assert L.ycrdt_docs_transact(d.engine._h, wr, 2, ctypes.byref(out), offs, codes, None) == E_ARG
        assert not out.ptr and out.len == 0
    assert d.encode_state_as_update() == before and d.take_local_update() == NOTHING
    # a null key and a bad value are the op's own failure and take no clock: the ops around them chain
    ups, codes, st = crdt_amd.docs_transact_stats([("map_set", d, "m", ("a", V)), ("map_set", d, "m", ("a", b"\xff")), ("map_set", d, "m", ("a", I1))])
    assert codes == [0, E_ARG, 0] and ups[1] == b"" and _stats(st) == (3, 0, 0, 1), (codes, st)
    t = _doc(7, _map_doc(), None)
    for op, arg in (("map_set", ("a", V)), ("map_set", ("a", I1))):
        code, want = _single(t, op, "m", arg, None)
        assert code == 0 and want == ups[0 if arg[1] == V else 2]


# ---------------------------------------------------------------- Yjs's recorded scripts
def _dependent_call(steps):
    """writes_independent's rule over the recorded steps of one call."""
    entries, lists, root_entries, parents = set(), set(), set(), set()
    for s in steps:
        pk = s.get("parent_key")
        if s["op"].startswith("map_"):
            k = (s["root"], pk, s["key"])
            if k in entries:
                return True
            entries.add(k)
            if pk is None:
                root_entries.add((s["root"], s["key"]))
        else:
            if (s["root"], pk) in lists:
                return True
            lists.add((s["root"], pk))
        if pk is not None:
            parents.add((s["root"], pk))
    return bool(root_entries & parents)


def test_recorded_scripts_in_calls_of_8():
    """The 60 recorded scripts as 60 documents. Between the recorded `apply` steps each script's
    consecutive local ops are cut into calls of at most 8 ops; round k issues every script's k-th
    event: the applies through one apply_updates_multi, the calls through ONE docs_transact. After it
    every document holds the state Yjs recorded behind the call's last op. (tests/test_write_chain.py
    plans the list chains of the ops_root_* scripts on the CPU and flags none of their ops, which
    is what the cap on ops_single below rests on: calls of 8, not of 4.)

    So that the test cannot pass on the fallback: of the ops of documents that are neither pending nor
    empty at their call at most 5 % may be ops_single, and at least 100 of the 164 dependent calls
    must have run wholly on the device. One docs_transact carries a round's calls of all scripts and
    reports one ops_chained, so a dependent call is counted when its round sent no op of an eligible
    document to the single calls and the round's ops_chained is at least the number of its dependent
    calls on eligible documents (each has at least one chained op)."""
    cases = _ops_cases()
    assert len(cases) == 60
    events = []  # per case: ("apply", step) | ("call", [steps])
    for c in cases:
        ev = []
        for s in c["steps"]:
            if s["op"] == "apply":
                ev.append(("apply", s))
            elif ev and ev[-1][0] == "call" and len(ev[-1][1]) < 8:
                ev[-1][1].append(s)
            else:
                ev.append(("call", [s]))
        events.append(ev)
    docs = [crdt_amd.Doc(client_id=c["client"]) for c in cases]
    touched = set()
    eligible = single = calls = dependent_calls = dependent_on_device = rounds_chained = 0
    for k in range(max(len(ev) for ev in events)):
        live = [(d, ev[k]) for d, ev in zip(docs, events) if k < len(ev)]
        applies = [(d, e[1]) for d, e in live if e[0] == "apply"]
        if applies:
            crdt_amd.apply_updates_multi([d for d, _ in applies], [bytes.fromhex(s["update"]) for _, s in applies])
            touched |= {id(d) for d, _ in applies}
        local = [(d, e[1]) for d, e in live if e[0] == "call"]
        if local:
            pending = [any(d.pending()) for d, _ in local]
            stateless = [not p and id(d) not in touched for (d, _), p in zip(local, pending)]
            ops = [_step_op(d, s) for d, steps in local for s in steps]
            ups, codes, st = crdt_amd.docs_transact_stats(ops)
            assert codes == [0] * len(ops), (k, codes)
            n_pending = sum(len(steps) for (_, steps), p in zip(local, pending) if p)
            n_empty = sum(len(steps) for (_, steps), e in zip(local, stateless) if e)
            assert st["ops_device"] + st["ops_single"] + st["ops_empty"] == len(ops) and st["ops_empty"] == n_empty and st["ops_single"] >= n_pending, (k, st)
            extra = st["ops_single"] - n_pending
            dep = sum(_dependent_call(steps) for (_, steps), p, e in zip(local, pending, stateless) if not p and not e)
            print(f"round {k}: {len(local)} calls, {len(ops)} ops, {dep} dependent calls on eligible documents, {st}")
            eligible += len(ops) - n_pending - n_empty
            single += extra
            calls += len(local)
            dependent_calls += sum(_dependent_call(steps) for _, steps in local)
            if not extra:  # every dependent call of an eligible document ran on the device: at least one chained op each
                assert st["ops_chained"] >= dep, (k, st, dep)
                dependent_on_device += dep
            rounds_chained += st["ops_chained"] > 0
            at = 0
            for d, steps in local:
                if any(ups[at:at + len(steps)]):
                    touched.add(id(d))
                at += len(steps)
        for d, e in live:
            last = e[1] if e[0] == "apply" else e[1][-1]
            assert d.encode_state_as_update().hex() == last["state"], (k, e[0])
    print(f"{calls} calls ({dependent_calls} dependent), {eligible} eligible ops, {single} of them single; "
          f"{dependent_on_device} dependent calls wholly on the device, {rounds_chained} rounds with chained ops")
    assert calls == 302 and dependent_calls == 164
    assert single * 20 <= eligible, (single, eligible)
    assert dependent_on_device >= 100, dependent_on_device
    for d, c in zip(docs, cases):
        assert json.loads(d.root_json("users", "map")) == c["json"]["users"], c["name"]
        assert json.loads(d.root_json("messages", "array")) == c["json"]["messages"], c["name"]
