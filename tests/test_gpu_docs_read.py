"""Point reads for many documents in one device pass (ycrdt_docs_read / crdt_amd.docs_read): YMap.get
/ size and YArray.get / length over the view of one multi-document merge, one lane per read
(yc_read.hip). Every answer must equal the per-document single call — Doc.map_get / map_size /
array_get / array_length, the host reads over the same view — byte for byte, and, where the fixtures
record it, Yjs 13.5.16's own toJSON().

The hand-written updates and their builders are those of tests/test_gpu_docs_json.py.
"""
import ctypes
import json
import os
import random

import pytest

crdt_amd = pytest.importorskip("crdt_amd")

from tests.test_gpu_docs_json import (ANY, SETS, STRING, TYPE, _alternating_list, _nested, _nested_json, _small_doc, any_int,  # noqa: E402
                                      any_str, anys, doc_of, item, update, vs, vu)
from tests.test_read_order import NAMES  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GETS = ("map_get", "array_get")


def single(rd):
    op, d, root, arg, pkey = (tuple(rd) + (None, None))[:5]
    if op == "map_get":
        return d.map_get(root, arg, parent_key=pkey)
    if op == "array_get":
        return d.array_get(root, arg, parent_key=pkey)
    return d.map_size(root, parent_key=pkey) if op == "map_size" else d.array_length(root, parent_key=pkey)


def ask(reads, engine=None):
    """docs_read over the reads: the stats add up and every answer is the single call's."""
    got, st = crdt_amd.docs_read_stats(reads, engine=engine)
    assert len(got) == len(reads)
    assert st["reads_device"] + st["reads_single"] + st["reads_empty"] == len(reads), st
    assert st["out_bytes"] == sum(len(g[1].encode()) for rd, g in zip(reads, got) if rd[0] in GETS)
    assert st["depth_max"] >= 4 and st["name_max"] >= 64
    for rd, g in zip(reads, got):
        assert g == single(rd), (rd[0], rd[2:], g)
        if rd[0] in GETS:
            assert g[0] in (0, 1, 2) and (g[0] == 1 or g[1] == "")
    return got, st


# ---------------------------------------------------------------- golden fleet
def _fleet_reads(cases, docs):
    """(read, what Yjs recorded) for every root of every case: each key, an absent key, each index,
    the index past the end, the size / length, and the reads of the other kind.

    YMap.size counts an entry whose value is `undefined`; JSON.stringify drops it from the recorded
    toJSON. So a map's size is the recorded key count plus its `undefined` entries, which are looked
    up among every key the fixtures use (state 2 of the single call)."""
    out = []
    universe = sorted({k for c in cases for root, kind in c["roots"].items() if kind == "map" for k in c["json"][root]} | {"u"})  # (kat_binary sets `u` to undefined: gen_fixtures.js)
    for c, d in zip(cases, docs):
        for root, kind in c["roots"].items():
            want = c["json"][root]
            if kind == "map":
                out += [(("map_get", d, root, k), ("value", v)) for k, v in want.items()]
                out.append((("map_get", d, root, "no such key é"), ("absent", None)))
                undefined = sum(1 for k in universe if k not in want and d.map_get(root, k)[0] == 2)
                out.append((("map_size", d, root), ("count", len(want) + undefined)))
                out.append((("array_length", d, root), ("count", 0)))
                out.append((("array_get", d, root, 0), ("absent", None)))
            else:
                out += [(("array_get", d, root, i), ("element", v)) for i, v in enumerate(want)]
                out.append((("array_get", d, root, len(want)), ("absent", None)))
                out.append((("array_length", d, root), ("count", len(want))))
                out.append((("map_size", d, root), ("count", 0)))
                out.append((("map_get", d, root, "k"), ("absent", None)))
    return out


def _check_recorded(pairs, got):
    for (rd, (what, want)), g in zip(pairs, got):
        if what == "count":
            assert g == want, (rd[0], rd[2:], g)
        elif what == "absent":
            assert g == (0, ""), (rd[0], rd[2:], g)
        elif what == "element" and g[0] == 2:  # an `undefined` element: toJSON records null, get returns undefined
            assert want is None and g[1] == ""
        else:
            assert g[0] == 1 and json.loads(g[1]) == want, (rd[0], rd[2:], g)


def test_golden_fleet(golden):
    cases = [c for s in SETS for c in golden[s]]
    assert len(cases) == 202 and sum(len(c["roots"]) for c in cases) == 441
    docs = [crdt_amd.Doc(client_id=0x7FFFFFF0) for _ in cases]
    idx, ups = [], []
    for i, c in enumerate(cases):
        for u in c["updates"]:
            idx.append(i)
            ups.append(bytes.fromhex(u))
    crdt_amd.apply_updates_multi(docs, ups, doc_index=idx)
    pairs = _fleet_reads(cases, docs)
    assert sum(1 for _, (w, _) in pairs if w == "value") == 985 and sum(1 for _, (w, _) in pairs if w == "element") == 4919
    random.Random(11).shuffle(pairs)
    got, st = ask([rd for rd, _ in pairs])
    assert st["reads_single"] == 0, st
    _check_recorded(pairs, got)


def test_recorded_op_scripts_final_states():
    """crdt.js's shape: root map `users` -> a value or one YArray per key, root array `messages`."""
    with open(os.path.join(HERE, "golden", "ops.json")) as f:
        cases = json.load(f)["cases"]
    docs = [doc_of(bytes.fromhex(c["steps"][-1]["state"])) for c in cases]
    pairs, nested, lists = [], 0, 0
    for c, d in zip(cases, docs):
        for k, v in c["json"]["users"].items():
            pairs.append((("map_get", d, "users", k), ("value", v)))
            if not isinstance(v, list):
                continue
            lists += 1
            if d.map_type_at("users", k) == 0:  # a nested YArray
                nested += 1
                pairs.append((("array_length", d, "users", None, k), ("count", len(v))))
                pairs += [(("array_get", d, "users", i, k), ("element", x)) for i, x in enumerate(v)]
                pairs.append((("array_get", d, "users", len(v), k), ("absent", None)))
            else:  # a plain array value: no shared type to read into
                pairs.append((("array_length", d, "users", None, k), ("count", 0)))
                pairs.append((("array_get", d, "users", 0, k), ("absent", None)))
            pairs.append((("map_size", d, "users", None, k), ("count", 0)))  # the other kind: empty
        pairs += [(("array_get", d, "messages", i), ("element", x)) for i, x in enumerate(c["json"]["messages"])]
    # 128 list-valued keys: 108 nested YArrays (the `list*` keys) and 20 plain arrays set as values
    assert lists == 128 and nested == 108 and sum(len(c["json"]["users"]) for c in cases) == 337
    assert sum(len(c["json"]["messages"]) for c in cases) == 998
    got, st = ask([rd for rd, _ in pairs])
    assert st["reads_single"] == 0, st
    _check_recorded(pairs, got)


# ---------------------------------------------------------------- request shapes
def test_request_shapes():
    d, e2 = _small_doc(), _small_doc(9)
    empty = crdt_amd.Doc(client_id=3)
    queued = crdt_amd.Doc(client_id=4)
    queued.apply_update(update(6, [(item(ANY, anys(any_int(9)), root="m", psub="q"), 1)]))  # not flushed
    reads = [("map_get", d, "m", "a"), ("map_get", d, "m", "a"), ("array_get", d, "l", 1), ("array_get", d, "l", 0),
             ("array_length", d, "l"), ("map_size", d, "m"), ("map_get", d, "nope", "a"), ("array_get", d, "nope", 0),
             ("map_size", d, "nope"), ("array_length", d, "nope"), ("map_get", d, "m", "a", "a"), ("array_length", d, "m", None, "zz"),
             ("map_get", empty, "m", "a"), ("array_length", empty, "l"), ("map_get", queued, "m", "q"), ("map_get", e2, "m", "a"),
             ("array_get", d, "l", 1)]
    got, st = ask(reads)
    assert got[:6] == [(1, "1"), (1, "1"), (1, "2"), (1, '"x"'), 2, 1]
    assert got[6:12] == [(0, ""), (0, ""), 0, 0, (0, ""), 0]
    assert got[12:] == [(0, ""), 0, (1, "9"), (1, "1"), (1, "2")]
    assert st["reads_empty"] == 2 and st["reads_single"] == 0 and st["reads_device"] == 15, st


def test_documents_sharing_clients_and_roots():
    from crdt_amd.workload import gen_map

    docs = [doc_of(*gen_map(n_keys=40, n_replicas=4, ops_per_replica=30, seed=300 + i)[0]) for i in range(3)]
    keys = sorted({k for d in docs for k in json.loads(d.root_json("users", "map"))})
    got, st = ask([("map_get", d, "users", k) for d in docs for k in keys] + [("map_size", d, "users") for d in docs])
    assert st["reads_single"] == 0, st
    assert len({tuple(got[i * len(keys):(i + 1) * len(keys)]) for i in range(3)}) == 3


def test_no_read_and_argument_errors():
    got, st = crdt_amd.docs_read_stats([])
    assert got == [] and st["out_bytes"] == 0 and st["reads_device"] == st["reads_single"] == st["reads_empty"] == 0
    d = _small_doc()
    other = crdt_amd.Engine()
    with pytest.raises(crdt_amd.YcrdtError):
        crdt_amd.docs_read([("map_get", d, "m", "a")], engine=other)  # a document of another engine
    with pytest.raises(ValueError):
        crdt_amd.docs_read([("map_has", d, "m", "a")])
    L = crdt_amd.lib()

    def call(doc, root, key, op):
        rd = (crdt_amd._Read * 1)()
        rd[0].doc, rd[0].root, rd[0].key, rd[0].op = doc, root, key, op
        out, offs = crdt_amd._Out(), (ctypes.c_uint64 * 2)()
        states, counts = (ctypes.c_int32 * 1)(), (ctypes.c_uint64 * 1)()
        rc = L.ycrdt_docs_read(d.engine._h, rd, 1, ctypes.byref(out), offs, states, counts, None)
        assert not out.ptr and out.len == 0
        return rc

    h = d._h.value
    for doc, root, key, op in ((None, b"m", b"a", 0), (h, None, b"a", 0), (h, b"m", None, 0), (h, b"m", b"a", 4), (h, b"m", b"a", -1)):
        assert call(doc, root, key, op) == -6  # YCRDT_E_ARG


# ---------------------------------------------------------------- scan and segment edges
@pytest.mark.parametrize("n", [255, 256, 257, 1025])
def test_elements_across_blocks(n):
    d = doc_of(_alternating_list(n))
    at = sorted({0, 254, 255, 256, n - 1, n} & set(range(n + 1)))
    got, st = ask([("array_get", d, "a", i) for i in at] + [("array_length", d, "a")])
    assert st["reads_device"] == len(at) + 1, st
    assert got[-1] == n
    for i, g in zip(at, got):
        want = None if i == n else i % 50 if i % 2 == 0 else chr(97 + i % 26)
        assert g == ((0, "") if i == n else (1, json.dumps(want)))


def test_struct_with_a_deleted_run():
    d = doc_of(update(21, [(item(ANY, anys(*[any_int(i % 60) for i in range(65)]), root="a"), 65)], deleted=[(20, 10)]))
    got, st = ask([("array_get", d, "a", i) for i in (19, 20, 54, 55)] + [("array_length", d, "a")])
    assert st["reads_device"] == 5, st
    live = [i % 60 for i in range(65) if not 20 <= i < 30]
    assert got == [(1, str(live[19])), (1, str(live[20])), (1, str(live[54])), (0, ""), 55]


# ---------------------------------------------------------------- values
def test_values_one_by_one():
    s = 'q"\n\U0001F600z'
    d = doc_of(update(22, [
        (item(STRING, vs(s), root="a"), len(s) + 1),  # (UTF-16 length: the astral character counts twice)
        (item(ANY, anys(bytes([127]), bytes([118, 1]) + vs("k") + bytes([117, 2, 127, 126])), origin=(22, len(s))), 2),
        (item(ANY, anys(bytes([127])), root="m", psub="gone"), 1),
        (item(ANY, anys(bytes([116, 2, 7, 255])), root="m", psub="bin"), 1),
    ]))
    n = d.array_length("a")
    got, st = ask([("array_get", d, "a", i) for i in range(n + 1)] + [("map_get", d, "m", "gone"), ("map_get", d, "m", "bin"),
                                                                      ("map_size", d, "m"), ("array_length", d, "a")])
    assert st["reads_single"] == 0, st  # the astral member included: the element is found as view_array_get finds it
    assert got[-4:] == [(2, ""), (1, '{"0":7,"1":255}'), 2, n]
    assert (2, "") in got[:n] and (1, '{"k":[null,null]}') in got[:n] and (1, '"q"') == got[0]

    c = 41
    t = doc_of(update(c, [
        (item(TYPE, vu(2), root="m", psub="text"), 1),
        (item(STRING, vs('he said "hi"\n'), parent=(c, 0)), 13),
        (item(STRING, vs("\U0001F600!"), origin=(c, 13)), 3),
        (item(TYPE, vu(3) + vs("div"), root="m", psub="xml"), 1),
        (item(TYPE, vu(2), root="m", psub="empty_text"), 1),
        (item(TYPE, vu(0), root="m", psub="empty_array"), 1),
        (item(TYPE, vu(1), root="m", psub="empty_map"), 1),
    ]))
    want = {"text": 'he said "hi"\n\U0001F600!', "xml": "", "empty_text": "", "empty_array": [], "empty_map": {}}
    got, st = ask([("map_get", t, "m", k) for k in want] + [("map_size", t, "m"), ("array_length", t, "m", None, "empty_array"),
                                                             ("map_size", t, "m", None, "empty_map"), ("array_get", t, "m", 0, "empty_array")])
    assert st["reads_single"] == 0, st
    assert [json.loads(g[1]) for g in got[:5]] == list(want.values()) and all(g[0] == 1 for g in got[:5])
    assert got[5:] == [5, 0, 0, (0, "")]


def test_a_value_inside_another_reads_value():
    """Two reads whose texts overlap — a nested type and a nested type inside it — cannot both be
    laid out by one placement: the outer one takes the single call, both answers are right."""
    c = 51
    d = doc_of(update(c, [
        (item(TYPE, vu(0), root="m", psub="outer"), 1),
        (item(TYPE, vu(1), parent=(c, 0)), 1),
        (item(ANY, anys(any_int(3)), parent=(c, 1), psub="x"), 1),
        (item(ANY, anys(any_str("tail")), origin=(c, 1)), 1),
    ]))
    got, st = ask([("map_get", d, "m", "outer"), ("array_get", d, "m", 0, "outer"), ("array_get", d, "m", 1, "outer")])
    assert got == [(1, '[{"x":3},"tail"]'), (1, '{"x":3}'), (1, '"tail"')]
    assert st["reads_single"] == 1 and st["reads_device"] == 2, st
    got, st = ask([("map_get", d, "m", "outer"), ("array_get", d, "m", 1, "outer")])
    assert st["reads_single"] == 0, st


# ---------------------------------------------------------------- names
def test_entry_names_and_the_name_bound():
    names = list(NAMES)
    random.Random(3).shuffle(names)
    short = [(item(ANY, anys(any_int(i % 60)), root="m", psub=n), 1) for i, n in enumerate(names)]
    d_short = doc_of(update(7, short))
    long_entry = b"b" * 64 + b"L" * 236
    d_long = doc_of(update(7, short + [(item(ANY, anys(any_int(5)), root="m", psub=long_entry), 1)]))
    askable = [n for n in names if b"\x00" not in n]  # (the C ABI takes NUL-terminated keys; every name here is UTF-8)
    assert len(askable) == len(names) - 2
    got, st = ask([("map_get", d_short, "m", n.decode()) for n in askable] + [("map_size", d_short, "m")])
    assert st["reads_single"] == 0, st
    assert got[:-1] == [(1, str(names.index(n) % 60)) for n in askable] and got[-1] == len(names)
    # a request past the bound, and an entry past the bound sharing the request's first 64 bytes
    got, st = ask([("map_get", d_short, "m", "L" * 300)])
    assert st["reads_single"] == 1 and got == [(0, "")], st
    got, st = ask([("map_get", d_long, "m", "b" * 64)])
    assert st["reads_single"] == 1 and got == [(1, str(names.index(b"b" * 64) % 60))], st
    got, st = ask([("map_get", d_short, "m", "b" * 64), ("map_get", d_long, "m", "b" * 63 + "a"), ("map_size", d_long, "m")])
    assert st["reads_single"] == 0 and got[2] == len(names) + 1, st


# ---------------------------------------------------------------- depth
def test_depth_bound():
    """`deep`.m is sized by the same sweeps that size the root `deep` for ycrdt_docs_json, so the
    read is on the device exactly where the root's toJSON is: with depth_max types below the root
    it is, with one more it takes the single call. The value itself then holds depth_max - 1 and
    depth_max nested levels: read as a value, the bound sits one level lower than the count of
    levels inside the text suggests."""
    dmax = crdt_amd.docs_read_stats([])[1]["depth_max"]
    at, past = doc_of(_nested(dmax)), doc_of(_nested(dmax + 1))
    got, st = ask([("map_get", at, "deep", "m"), ("map_get", at, "deep", "flat")])
    assert st["reads_device"] == 2 and st["reads_single"] == 0, st
    assert json.loads(got[0][1]) == _nested_json(dmax)["m"] and got[1] == (1, "1")
    got, st = ask([("map_get", past, "deep", "m"), ("map_get", past, "deep", "flat"), ("map_get", at, "deep", "m")])
    assert st["reads_device"] == 2 and st["reads_single"] == 1, st
    assert json.loads(got[0][1]) == _nested_json(dmax + 1)["m"] and got[1] == (1, "1")


# ---------------------------------------------------------------- several passes, routing
def test_several_device_passes(monkeypatch, golden):
    cases = [c for s in SETS for c in golden[s]][:40]
    docs = [doc_of(*[bytes.fromhex(u) for u in c["updates"]]) for c in cases]
    reads = [rd for rd, _ in _fleet_reads(cases, docs)]
    random.Random(5).shuffle(reads)
    one, st1 = ask(reads)
    monkeypatch.setenv("YCRDT_DOCS_READ_PASS_BYTES", "600")
    many, st = ask(reads)
    assert many == one and st["reads_single"] == 0 and st["reads_device"] == st1["reads_device"], st
    monkeypatch.setenv("YCRDT_DOCS_READ_PASS_BYTES", "1")  # one document per pass
    many, st = ask(reads)
    assert many == one and st["reads_single"] == 0, st


def test_routing_pending_compat_and_switch(monkeypatch):
    with open(os.path.join(HERE, "golden", "pending.json")) as f:
        gap = next(c for c in json.load(f)["cases"] if c["name"] == "kat_gap")
    pend = crdt_amd.Doc(client_id=0x7FFFFFF0)
    pend.apply_update(bytes.fromhex(gap["updates"][0]))
    assert pend.pending()[0]
    d = _small_doc()
    got, st = ask([("map_size", pend, "m"), ("map_get", d, "m", "a")])
    assert st["reads_single"] == 1 and st["reads_device"] == 1, st
    assert got[0] == len(gap["steps"][0]["json"]["m"])
    pend.apply_update(bytes.fromhex(gap["updates"][1]))
    full = gap["steps"][1]["json"]["m"]
    got, st = ask([("map_size", pend, "m")] + [("map_get", pend, "m", k) for k in full])
    assert st["reads_device"] == 1 + len(full) and got[0] == len(full), st
    assert [json.loads(g[1]) for g in got[1:]] == list(full.values())

    e135 = crdt_amd.Engine(compat=135)
    old = doc_of(update(5, [(item(ANY, anys(any_int(1)), root="m", psub="a"), 1)]), engine=e135)
    got, st = ask([("map_get", old, "m", "a")], engine=e135)
    assert st["reads_single"] == 1 and st["reads_device"] == 0 and got == [(1, "1")]

    reads = [("map_get", d, "m", "a"), ("array_get", d, "l", 0), ("array_length", d, "l"), ("map_size", d, "m")]
    monkeypatch.setenv("YCRDT_DOCS_READ", "0")
    got, st = ask(reads)
    assert st["reads_single"] == 4 and st["reads_device"] == 0 and got == [(1, "1"), (1, '"x"'), 2, 1]
    monkeypatch.delenv("YCRDT_DOCS_READ")
    got, st = ask(reads)
    assert st["reads_single"] == 0 and st["reads_device"] == 4 and got == [(1, "1"), (1, '"x"'), 2, 1]
