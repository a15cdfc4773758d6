"""Root toJSON for many documents in one device pass (ycrdt_docs_json / crdt_amd.docs_json): the
distinct documents' resident states merged as one multi-document batch, the view over it, and the
JSON text sized, laid out and written on the device (yc_json.hip). Every answer must be byte-identical
to the per-document Doc.root_json — the host writer over the same view — and, where the fixtures
record it, equal to Yjs 13.5.16's own toJSON().

The equality with Doc.root_json is a consistency check, not a reference: both writers are built
from the same yc_json.h, so a wrong digit, escape or comma there passes on both sides, and the
json.loads comparisons are blind to the text form. What holds the text itself — Node's bytes, an
exact number reference and the host build under sanitizers — is tests/test_gpu_json_values.py
with tests/test_num_text.py and tests/test_jsnum_reference.py.

Hand-written updates (Yjs v1 wire format, one client each) build the shapes the fixtures lack: entry
names that stress the ordering, lists that cross the 256-lane blocks of the scans, types nested to
the device path's depth bound and one level past it.
"""
import json
import os
import random

import pytest

crdt_amd = pytest.importorskip("crdt_amd")

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SETS = ("kat", "map", "array", "nested")


# ---------------------------------------------------------------- hand-written updates
def vu(n):
    out = bytearray()
    while n > 127:
        out.append(128 | (n & 127))
        n >>= 7
    out.append(n)
    return bytes(out)


def vs(b):
    b = b if isinstance(b, bytes) else b.encode()
    return vu(len(b)) + b


ANY, STRING, TYPE = 8, 4, 7


def item(ref, content, root=None, parent=None, origin=None, psub=None):
    """One Item: origin (client, clock), or a parent — root name / parent item id — and a parentSub."""
    info = ref | (0x80 if origin else 0) | (0x20 if psub is not None and not origin else 0)
    out = bytes([info])
    if origin:
        out += vu(origin[0]) + vu(origin[1])
    else:
        out += (vu(1) + vs(root)) if parent is None else (vu(0) + vu(parent[0]) + vu(parent[1]))
        if psub is not None:
            out += vs(psub)
    return out + content


def update(client, items, deleted=()):
    """items: (bytes, clock length) in clock order from 0; deleted: (clock, len) ranges of the client."""
    out = vu(1) + vu(len(items)) + vu(client) + vu(0) + b"".join(b for b, _ in items)
    if deleted:
        out += vu(1) + vu(client) + vu(len(deleted)) + b"".join(vu(c) + vu(n) for c, n in deleted)
    else:
        out += vu(0)
    return out


def anys(*values):
    return vu(len(values)) + b"".join(values)


def any_int(n):
    assert 0 <= n < 64
    return bytes([125, n])


def any_str(s):
    return bytes([119]) + vs(s)


def doc_of(*updates, engine=None):
    d = crdt_amd.Doc(client_id=0x7FFFFFF0, engine=engine)
    d.apply_updates(list(updates))
    d.flush()
    return d


def ask(reqs, engine=None):
    """docs_json over (doc, root, kind) requests: every text equals the per-document root_json."""
    texts, st = crdt_amd.docs_json_stats([d for d, _, _ in reqs], [r for _, r, _ in reqs], [k for _, _, k in reqs], engine=engine)
    assert len(texts) == len(reqs)
    assert st["pairs_device"] + st["pairs_single"] + st["pairs_empty"] == len(reqs), st
    assert st["out_bytes"] == sum(len(t.encode()) for t in texts)
    assert st["depth_max"] >= 4 and st["name_max"] >= 64
    for (d, root, kind), t in zip(reqs, texts):
        assert t == d.root_json(root, kind), (root, kind, t[:200])
    return texts, st


# ---------------------------------------------------------------- golden fleet
@pytest.fixture(scope="module")
def fleet_cases(golden):
    cases = [c for s in SETS for c in golden[s]]
    assert len(cases) == 202 and sum(len(c["roots"]) for c in cases) == 441
    return cases


def _golden_check(cases, docs):
    reqs = [(d, root, kind) for c, d in zip(cases, docs) for root, kind in c["roots"].items()]
    want = [c["json"][root] for c in cases for root in c["roots"]]
    for order in (list(range(len(reqs))), random.Random(7).sample(range(len(reqs)), len(reqs))):
        texts, st = ask([reqs[i] for i in order])
        assert st["pairs_single"] == 0, st
        assert st["pairs_device"] + st["pairs_empty"] == len(reqs)
        for i, t in zip(order, texts):
            assert json.loads(t) == want[i], (i, reqs[i][1])


def test_golden_fleet_flushed_one_by_one(fleet_cases):
    docs = []
    for c in fleet_cases:
        d = crdt_amd.Doc(client_id=0x7FFFFFF0)
        d.apply_updates([bytes.fromhex(u) for u in c["updates"]])
        d.flush()
        docs.append(d)
    _golden_check(fleet_cases, docs)


def test_golden_fleet_ingested_together(fleet_cases):
    docs = [crdt_amd.Doc(client_id=0x7FFFFFF0) for _ in fleet_cases]
    idx, ups = [], []
    for i, c in enumerate(fleet_cases):
        for u in c["updates"]:
            idx.append(i)
            ups.append(bytes.fromhex(u))
    crdt_amd.apply_updates_multi(docs, ups, doc_index=idx)
    _golden_check(fleet_cases, docs)


def test_recorded_op_scripts_final_states():
    """The final states of the recorded op scripts: root map -> one YArray per key (crdt.js's shape)."""
    with open(os.path.join(HERE, "golden", "ops.json")) as f:
        cases = json.load(f)["cases"]
    docs = [doc_of(bytes.fromhex(c["steps"][-1]["state"])) for c in cases]
    reqs = [(d, root, kind) for d in docs for root, kind in (("users", "map"), ("messages", "array"))]
    texts, st = ask(reqs)
    assert st["pairs_single"] == 0, st
    for k, c in enumerate(cases):
        assert json.loads(texts[2 * k]) == c["json"]["users"], c["name"]
        assert json.loads(texts[2 * k + 1]) == c["json"]["messages"], c["name"]
    assert any(isinstance(v, list) and v for c in cases for v in c["json"]["users"].values())  # nested arrays are there


# ---------------------------------------------------------------- request shapes
def _small_doc(client=5):
    return doc_of(update(client, [
        (item(ANY, anys(any_int(1)), root="m", psub="a"), 1),
        (item(ANY, anys(any_str("x"), any_int(2)), root="l"), 2),
    ]))


def test_request_shapes():
    d, e2 = _small_doc(), _small_doc(9)
    empty = crdt_amd.Doc(client_id=3)
    queued = crdt_amd.Doc(client_id=4)
    queued.apply_update(update(6, [(item(ANY, anys(any_int(9)), root="m", psub="q"), 1)]))  # not flushed
    reqs = [(d, "m", "map"), (d, "m", "map"), (d, "m", "array"), (d, "l", "map"), (d, "l", "array"), (d, "nope", "map"),
            (d, "nope", "array"), (empty, "m", "map"), (empty, "l", "array"), (queued, "m", "map"), (e2, "m", "map"), (d, "l", "array")]
    texts, st = ask(reqs)
    assert texts[:7] == ['{"a":1}', '{"a":1}', "[]", "{}", '["x",2]', "{}", "[]"]
    assert texts[7:] == ["{}", "[]", '{"q":9}', '{"a":1}', '["x",2]']
    assert st["pairs_empty"] == 2 and st["pairs_single"] == 0 and st["pairs_device"] == 10


def test_no_request_and_argument_errors():
    import ctypes

    texts, st = crdt_amd.docs_json_stats([], [], [])
    assert texts == [] and st["out_bytes"] == 0 and st["pairs_device"] == st["pairs_single"] == st["pairs_empty"] == 0
    d = _small_doc()
    other = crdt_amd.Engine()
    with pytest.raises(crdt_amd.YcrdtError):
        crdt_amd.docs_json([d], ["m"], ["map"], engine=other)  # a document of another engine
    with pytest.raises(ValueError):
        crdt_amd.docs_json([d], ["m"], ["text"])
    L = crdt_amd.lib()
    hs = (ctypes.c_void_p * 1)(d._h.value)
    out, offs = crdt_amd._Out(), (ctypes.c_uint64 * 2)()
    names = (ctypes.c_char_p * 1)(b"m")
    null_names = (ctypes.c_char_p * 1)(None)
    for nm, kinds in ((names, (ctypes.c_int * 1)(2)), (names, (ctypes.c_int * 1)(-1)), (null_names, (ctypes.c_int * 1)(0))):
        assert L.ycrdt_docs_json(d.engine._h, hs, nm, kinds, 1, ctypes.byref(out), offs, None) == -6  # YCRDT_E_ARG
        assert not out.ptr and out.len == 0


# ---------------------------------------------------------------- entry order
def test_entry_order_and_long_name():
    """Names sharing 8-, 16- and 40-byte prefixes, differing only in length, holding bytes >= 0x80,
    "a" beside "a\\0": the device orders them as HostView::index does. A 300-byte name is past the
    ordering's bound: that request takes the single path, the same map without it the device."""
    p8, p16, p40 = b"01234567", b"0123456789abcdef", b"z" * 40
    names = [p8 + b"B", p8 + b"A", p8, p16 + b"\xc3\xa9", p16 + b"e", p16, p40 + b"2", p40 + b"10", p40, b"a", b"a\x00", b"a\x00\x00",
             b"", b"\xf0\x9f\x98\x80", b"\xc3\xbf", b"\x7f", b"b" * 64, b"b" * 63 + b"a", b"b" * 64 + b"!"[:0]]
    names = list(dict.fromkeys(names))
    random.Random(3).shuffle(names)
    short = [(item(ANY, anys(any_int(i % 60)), root="m", psub=n), 1) for i, n in enumerate(names)]
    d_short = doc_of(update(7, short))
    d_long = doc_of(update(7, short + [(item(ANY, anys(any_int(5)), root="m", psub=b"L" * 300), 1)]))
    texts, st = ask([(d_short, "m", "map"), (d_long, "m", "map")])
    assert st["pairs_device"] == 1 and st["pairs_single"] == 1, st
    keys = list(json.loads(texts[0]).keys())
    assert keys == [n.decode() for n in sorted(names)]  # name bytes ascending, a prefix first
    assert len(json.loads(texts[1])) == len(names) + 1


# ---------------------------------------------------------------- scan and segment edges
def _alternating_list(n, root="a", client=11):
    """n single-element structs that cannot merge (ContentAny and ContentString alternate)."""
    items = []
    for i in range(n):
        ref, content = (ANY, anys(any_int(i % 50))) if i % 2 == 0 else (STRING, vs(chr(97 + i % 26)))
        items.append((item(ref, content, root=root) if i == 0 else item(ref, content, origin=(client, i - 1)), 1))
    return update(client, items)


@pytest.mark.parametrize("n", [255, 256, 257, 1000, 1025])
def test_list_members_across_blocks(n):
    d = doc_of(_alternating_list(n))
    texts, st = ask([(d, "a", "array")])
    assert st["pairs_device"] == 1
    got = json.loads(texts[0])
    assert got == [i % 50 if i % 2 == 0 else chr(97 + i % 26) for i in range(n)]


def test_segment_edges():
    # a 65-value ContentAny struct with a run deleted from its middle
    d1 = doc_of(update(21, [(item(ANY, anys(*[any_int(i % 60) for i in range(65)]), root="a"), 65)], deleted=[(20, 10)]))
    # a ContentString member with an astral character, a quote and a newline; undefined and nested values
    s = 'q"\n\U0001F600z'
    d2 = doc_of(update(22, [
        (item(STRING, vs(s), root="a"), len(s) + 1),  # (UTF-16 length: the astral character counts twice)
        (item(ANY, anys(bytes([127]), bytes([118, 1]) + vs("k") + bytes([117, 2, 127, 126])), origin=(22, len(s))), 2),
        (item(ANY, anys(bytes([127])), root="m", psub="gone"), 1),
        (item(ANY, anys(bytes([116, 2, 7, 255])), root="m", psub="bin"), 1),
    ]))
    texts, st = ask([(d1, "a", "array"), (d2, "a", "array"), (d2, "m", "map")])
    assert st["pairs_device"] == 3, st
    assert json.loads(texts[0]) == [i % 60 for i in range(65) if not 20 <= i < 30]
    assert json.loads(texts[1]) == ["q", '"', "\n", "\U0001F600", "z", None, {"k": [None, None]}]
    assert texts[2] == '{"bin":{"0":7,"1":255}}'


def test_documents_sharing_clients_and_roots():
    from crdt_amd.workload import gen_map

    docs = [doc_of(*gen_map(n_keys=40, n_replicas=4, ops_per_replica=30, seed=300 + i)[0]) for i in range(3)]
    texts, st = ask([(d, "users", "map") for d in docs] + [(docs[1], "users", "map")])
    assert st["pairs_device"] == 4, st
    assert len({texts[0], texts[1], texts[2]}) == 3 and texts[3] == texts[1]


def test_several_device_passes(monkeypatch, fleet_cases):
    """More resident state than one pass takes is split into several passes (2 GiB each; shrunk here
    to a few hundred bytes): documents in call order, every request answered by its document's pass."""
    cases = fleet_cases[:40]
    docs = [doc_of(*[bytes.fromhex(u) for u in c["updates"]]) for c in cases]
    reqs = [(d, root, kind) for c, d in zip(cases, docs) for root, kind in c["roots"].items()]
    random.Random(5).shuffle(reqs)
    one, st1 = ask(reqs)
    monkeypatch.setenv("YCRDT_DOCS_JSON_PASS_BYTES", "600")
    many, st = ask(reqs)
    assert many == one and st["pairs_single"] == 0 and st["pairs_device"] == st1["pairs_device"], st
    monkeypatch.setenv("YCRDT_DOCS_JSON_PASS_BYTES", "1")  # one document per pass
    many, st = ask(reqs)
    assert many == one and st["pairs_single"] == 0, st


# ---------------------------------------------------------------- depth
def _nested(levels, client=31):
    """root map "deep" -> `levels` shared types below it (YMaps, the innermost a YArray) -> values."""
    items = []
    for k in range(levels):
        tref = 0 if k == levels - 1 else 1
        where = dict(root="deep") if k == 0 else dict(parent=(client, k - 1))
        items.append((item(TYPE, vu(tref), psub="m", **where), 1))
    items.append((item(ANY, anys(any_int(7), any_str("leaf")), parent=(client, levels - 1)), 2))
    items.append((item(ANY, anys(any_int(1)), root="deep", psub="flat"), 1))
    return update(client, items)


def _nested_json(levels):
    v = [7, "leaf"]
    for _ in range(levels):
        v = {"m": v}
    v["flat"] = 1
    return v


def test_depth_bound():
    dmax = crdt_amd.docs_json_stats([], [], [])[1]["depth_max"]
    at, past = doc_of(_nested(dmax)), doc_of(_nested(dmax + 1))
    texts, st = ask([(at, "deep", "map")])
    assert st["pairs_device"] == 1 and st["pairs_single"] == 0, st
    assert json.loads(texts[0]) == _nested_json(dmax)
    texts, st = ask([(past, "deep", "map"), (at, "deep", "map")])
    assert st["pairs_device"] == 1 and st["pairs_single"] == 1, st
    assert json.loads(texts[0]) == _nested_json(dmax + 1)


def test_nested_text_and_xml():
    c = 41
    d = doc_of(update(c, [
        (item(TYPE, vu(2), root="m", psub="text"), 1),
        (item(STRING, vs('he said "hi"\n'), parent=(c, 0)), 13),
        (item(STRING, vs("\U0001F600!"), origin=(c, 13)), 3),
        (item(TYPE, vu(3) + vs("div"), root="m", psub="xml"), 1),
        (item(TYPE, vu(2), root="m", psub="empty_text"), 1),
        (item(TYPE, vu(0), root="m", psub="empty_array"), 1),
        (item(TYPE, vu(1), root="m", psub="empty_map"), 1),
    ]))
    texts, st = ask([(d, "m", "map")])
    assert st["pairs_device"] == 1, st
    assert json.loads(texts[0]) == {"text": 'he said "hi"\n\U0001F600!', "xml": "", "empty_text": "", "empty_array": [], "empty_map": {}}


# ---------------------------------------------------------------- routing
def test_routing_pending_compat_and_switch(monkeypatch):
    with open(os.path.join(HERE, "golden", "pending.json")) as f:
        gap = next(c for c in json.load(f)["cases"] if c["name"] == "kat_gap")
    pend = crdt_amd.Doc(client_id=0x7FFFFFF0)
    pend.apply_update(bytes.fromhex(gap["updates"][0]))
    assert pend.pending()[0]
    d = _small_doc()
    texts, st = ask([(pend, "m", "map"), (d, "m", "map")])
    assert st["pairs_single"] == 1 and st["pairs_device"] == 1, st
    assert json.loads(texts[0]) == gap["steps"][0]["json"]["m"]
    pend.apply_update(bytes.fromhex(gap["updates"][1]))
    texts, st = ask([(pend, "m", "map")])
    assert st["pairs_device"] == 1 and json.loads(texts[0]) == gap["steps"][1]["json"]["m"]

    e135 = crdt_amd.Engine(compat=135)
    old = doc_of(update(5, [(item(ANY, anys(any_int(1)), root="m", psub="a"), 1)]), engine=e135)
    texts, st = ask([(old, "m", "map")], engine=e135)
    assert st["pairs_single"] == 1 and st["pairs_device"] == 0 and texts == ['{"a":1}']

    monkeypatch.setenv("YCRDT_DOCS_JSON", "0")
    texts, st = ask([(d, "m", "map"), (d, "l", "array")])
    assert st["pairs_single"] == 2 and st["pairs_device"] == 0 and texts == ['{"a":1}', '["x",2]']
    monkeypatch.delenv("YCRDT_DOCS_JSON")
    texts, st = ask([(d, "m", "map"), (d, "l", "array")])
    assert st["pairs_single"] == 0 and st["pairs_device"] == 2 and texts == ['{"a":1}', '["x",2]']
