"""The cache refresh for many documents in one device pass (ycrdt_docs_cache / crdt_amd.docs_cache):
for every document the text of crdt.js's cache object `c`, one member per live entry of the
document's index map, each the toJSON of the root the entry names — the index read on the device
(yc_cache.hip) over the sorted view keys of one multi-document merge.

The reference is Yjs 13.5.16: tests/golden/cache.json records, for small documents that cover the
index values, names and histories that matter, the object crdt.js's own loop builds; json.loads of
every answer must equal it. On top of that every answer must be byte-identical to the composition
of per-document Doc.root_json calls in the index's member order. That second check is a consistency
check, not a reference (both sides are built from yc_json.h and yc_cache.h); what pins the kind rule
and the name text to Node is tests/test_index_kind.py.

Hand-written updates (Yjs v1 wire format) build the shapes the fixture lacks: indexes whose live
entries cross a wavefront and a 256-lane block with deleted entries in between, documents that
share client ids and root names, roots nested to the device path's depth bound and one past it.
"""
import json
import random

import pytest

crdt_amd = pytest.importorskip("crdt_amd")

from tests.cache_fixture import cases as fixture_cases, updates as fixture_updates  # noqa: E402

pytestmark = pytest.mark.gpu


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


ANY, TYPE = 8, 7


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


def update(client, items, deleted=(), clock=0):
    """items: (bytes, clock length) in clock order from `clock`; deleted: (clock, len) ranges of the client."""
    out = vu(1) + vu(len(items)) + vu(client) + vu(clock) + b"".join(b for b, _ in items)
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


def doc_of(*ups, engine=None):
    d = crdt_amd.Doc(client_id=0x7FFFFFF0, engine=engine)
    d.apply_updates(list(ups))
    d.flush()
    return d


# ---------------------------------------------------------------- the helper every call goes through
def loosely_map(v):
    """JavaScript's `v == 'map'` for a value that went through JSON"""
    while isinstance(v, list) and len(v) == 1:
        v = v[0]
    return v == "map"


def compose(d, index="ix", undefined=()):
    """`c` from per-document calls: the index's live entries (its JSON's members and the ones whose
    value is undefined, which that JSON drops) in the engine's member order, each through root_json."""
    ix = json.loads(d.root_json(index, "map"))
    names = sorted(set(ix) | set(undefined), key=lambda n: n.encode())
    return "{" + ",".join(json.dumps(n, ensure_ascii=False) + ":" + d.root_json(n, "map" if n in ix and loosely_map(ix[n]) else "array")
                          for n in names) + "}"


def ask(docs, index="ix", undefined=None, want=None, engine=None):
    """docs_cache over docs. undefined: {position: names of index entries whose value is undefined};
    want: {position: the object Yjs built}."""
    texts, st = crdt_amd.docs_cache_stats(docs, index, engine=engine)
    assert len(texts) == len(docs)
    assert st["docs_device"] + st["docs_single"] + st["docs_empty"] == len(docs), st
    assert st["out_bytes"] == sum(len(t.encode()) for t in texts)
    assert st["depth_max"] >= 4 and st["name_max"] >= 64
    for i, (d, t) in enumerate(zip(docs, texts)):
        assert t == compose(d, index, (undefined or {}).get(i, ())), (i, t[:300])
        if want and i in want:
            assert json.loads(t) == want[i], (i, t[:300])
    return texts, st


# ---------------------------------------------------------------- the fixture fleet
def _undefined_names(c):
    return [e["name"] for e in c["entries"] if e["content"] == "017f"]


def _fleet_check(docs):
    cs = fixture_cases()
    n65 = next(i for i, c in enumerate(cs) if c["name"] == "name_65")
    basic = next(i for i, c in enumerate(cs) if c["name"] == "basic")
    for order in (list(range(len(cs))) + [basic], random.Random(11).sample(range(len(cs)), len(cs)) + [basic]):
        want = {k: cs[i]["c"] for k, i in enumerate(order) if cs[i]["index"] == "ix"}
        undefined = {k: _undefined_names(cs[i]) for k, i in enumerate(order) if cs[i]["index"] == "ix"}
        texts, st = ask([docs[i] for i in order], undefined=undefined, want=want)
        assert st["docs_single"] == 1, st  # the 65-byte name, and only that document
        assert order.count(n65) == 1 and st["docs_device"] >= len(cs) - 2
        assert st["roots"] == sum(len(cs[i]["ix_keys"]) for i in set(order) if i != n65 and cs[i]["index"] == "ix") + \
            sum(1 for i in set(order) if cs[i]["index"] != "ix")  # (a repeated document once; the other index's document lists one decoy in `ix`)
        assert texts[-1] == texts[order.index(basic)]
    # the document whose index root has another name
    k = next(i for i, c in enumerate(cs) if c["index"] != "ix")
    texts, st = ask([docs[k], docs[basic]], index=cs[k]["index"], want={0: cs[k]["c"], 1: {}})
    assert st["docs_device"] == 2 and texts[1] == "{}", st


def test_fixture_fleet_flushed_one_by_one():
    _fleet_check([doc_of(*fixture_updates(c)) for c in fixture_cases()])


def test_fixture_fleet_ingested_together():
    cs = fixture_cases()
    docs = [crdt_amd.Doc(client_id=0x7FFFFFF0) for _ in cs]
    idx, ups = [], []
    for i, c in enumerate(cs):
        for u in fixture_updates(c):
            idx.append(i)
            ups.append(u)
    crdt_amd.apply_updates_multi(docs, ups, doc_index=idx)
    _fleet_check(docs)


# ---------------------------------------------------------------- ranks across wavefronts and blocks
def _indexed_doc(n_live, client):
    """An index with n_live live entries and a deleted one after every third; entry i names root
    r<i>, every other one as a map; some roots hold an entry or two list members, some nothing."""
    items, deleted, want = [], [], {}
    clock = 0

    def put(b, n=1):
        nonlocal clock
        items.append((b, n))
        clock += n

    i = 0
    while len(want) < n_live:
        name = "r%04d" % i
        is_map = i % 2 == 0
        put(item(ANY, anys(any_str("map" if is_map else "array")), root="ix", psub=name))
        want[name] = {} if is_map else []
        if i % 5 == 0:
            if is_map:
                put(item(ANY, anys(any_int(i % 60)), root=name, psub="k"))
                want[name] = {"k": i % 60}
            else:
                put(item(ANY, anys(any_int(i % 60), any_str(name)), root=name), 2)
                want[name] = [i % 60, name]
        if i % 3 == 2:  # a deleted entry sorts between the live ones
            put(item(ANY, anys(any_str("map")), root="ix", psub=name + "x"))
            deleted.append((clock - 1, 1))
        i += 1
    if not items:  # an index that lost its only entry
        put(item(ANY, anys(any_str("map")), root="ix", psub="gone"))
        deleted.append((0, 1))
    return update(client, items, deleted), want


def test_ranks_across_wavefronts_and_blocks():
    sizes = [0, 1, 63, 64, 65, 256, 257]
    built = [_indexed_doc(n, 50 + k) for k, n in enumerate(sizes)]
    docs = [doc_of(u) for u, _ in built]
    texts, st = ask(docs, want={k: w for k, (_, w) in enumerate(built)})
    assert st["docs_device"] == len(sizes) and st["docs_single"] == 0, st
    assert st["roots"] == sum(sizes)
    assert texts[0] == "{}"
    for n, t in zip(sizes, texts):
        assert list(json.loads(t)) == ["r%04d" % i for i in range(n)]  # member order: name bytes ascending
    one_by_one = [ask([d])[0][0] for d in docs[:4]]
    assert one_by_one == texts[:4]


def test_documents_sharing_clients_and_roots():
    def one(v):
        return update(7, [
            (item(ANY, anys(any_str("map")), root="ix", psub="m"), 1),
            (item(ANY, anys(any_str("array")), root="ix", psub="l"), 1),
            (item(ANY, anys(any_int(v)), root="m", psub="a"), 1),
            (item(ANY, anys(any_int(v + 1), any_int(v + 2)), root="l"), 2),
        ])

    docs = [doc_of(one(1)), crdt_amd.Doc(client_id=3), doc_of(one(10)), crdt_amd.Doc(client_id=4), doc_of(one(20))]
    texts, st = ask(docs)
    assert texts == ['{"l":[2,3],"m":{"a":1}}', "{}", '{"l":[11,12],"m":{"a":10}}', "{}", '{"l":[21,22],"m":{"a":20}}']
    assert st["docs_device"] == 3 and st["docs_empty"] == 2 and st["roots"] == 6, st


# ---------------------------------------------------------------- two root names in one hash slot
def _slot(name):
    """the 31 bits of FNV-1a the root group keys keep of a root name"""
    h = 2166136261
    for b in name.encode():
        h = ((h ^ b) * 16777619) & 0xFFFFFFFF
    return h >> 1


def test_root_names_sharing_a_hash_slot():
    """A listed root whose hash slot also holds another root's keys, and a listed root that is absent
    while another name fills its slot: the device tells by the names and hands the document over."""
    (a, b), (absent, other) = ("tzkfwtu", "snzyulw"), ("lsexqzd", "ztxtxde")
    assert _slot(a) == _slot(b) and _slot(absent) == _slot(other)
    mixed = doc_of(update(61, [
        (item(ANY, anys(any_str("map")), root="ix", psub=a), 1),
        (item(ANY, anys(any_int(1)), root=a, psub="mine"), 1),
        (item(ANY, anys(any_int(2)), root=b, psub="foreign"), 1),
    ]))
    lone = doc_of(update(62, [
        (item(ANY, anys(any_str("map")), root="ix", psub=absent), 1),
        (item(ANY, anys(any_int(3)), root=other, psub="foreign"), 1),
    ]))
    both = doc_of(update(63, [
        (item(ANY, anys(any_str("map")), root="ix", psub=a), 1),
        (item(ANY, anys(any_str("map")), root="ix", psub=b), 1),
        (item(ANY, anys(any_int(4)), root=a, psub="ka"), 1),
        (item(ANY, anys(any_int(5)), root=b, psub="kb"), 1),
    ]))
    texts, st = ask([mixed, _small(), lone, both])
    assert texts == ['{"%s":{"mine":1}}' % a, '{"m":{"a":1}}', '{"%s":{}}' % absent, '{"%s":{"kb":5},"%s":{"ka":4}}' % (b, a)]
    assert st["docs_single"] == 3 and st["docs_device"] == 1 and st["roots"] == 1, st


# ---------------------------------------------------------------- depth
def _nested(levels, client=31):
    """ix lists root map "deep" -> `levels` shared types below it (YMaps, the innermost a YArray) -> values."""
    items = []
    for k in range(levels):
        tref = 0 if k == levels - 1 else 1
        where = dict(root="deep") if k == 0 else dict(parent=(client, k - 1))
        items.append((item(TYPE, vu(tref), psub="m", **where), 1))
    items.append((item(ANY, anys(any_int(7), any_str("leaf")), parent=(client, levels - 1)), 2))
    items.append((item(ANY, anys(any_int(1)), root="deep", psub="flat"), 1))
    items.append((item(ANY, anys(any_str("map")), root="ix", psub="deep"), 1))
    items.append((item(ANY, anys(any_str("array")), root="ix", psub="other"), 1))
    return update(client, items)


def _nested_json(levels):
    v = [7, "leaf"]
    for _ in range(levels):
        v = {"m": v}
    v["flat"] = 1
    return {"deep": v, "other": []}


def test_depth_bound():
    dmax = crdt_amd.docs_cache_stats([])[1]["depth_max"]
    at, past = doc_of(_nested(dmax)), doc_of(_nested(dmax + 1))
    texts, st = ask([at], want={0: _nested_json(dmax)})
    assert st["docs_device"] == 1 and st["docs_single"] == 0, st
    texts, st = ask([past, at, at], want={0: _nested_json(dmax + 1), 1: _nested_json(dmax)})
    assert st["docs_device"] == 2 and st["docs_single"] == 1 and st["roots"] == 2, st


# ---------------------------------------------------------------- routing
def _small(v=1, client=5, engine=None):
    return doc_of(update(client, [
        (item(ANY, anys(any_str("map")), root="ix", psub="m"), 1),
        (item(ANY, anys(any_int(v)), root="m", psub="a"), 1),
    ]), engine=engine)


def test_routing_pending_compat_and_switch(monkeypatch):
    d = _small()
    pend = _small(2)
    pend.apply_update(update(77, [(item(ANY, anys(any_int(9)), root="m", psub="late"), 1)], clock=3))  # clocks 0..2 are missing
    assert pend.pending()[0]
    texts, st = ask([pend, d])
    assert texts == ['{"m":{"a":2}}', '{"m":{"a":1}}']
    assert st["docs_single"] == 1 and st["docs_device"] == 1, st

    e135 = crdt_amd.Engine(compat=135)
    old = _small(3, engine=e135)
    texts, st = ask([old], engine=e135)
    assert st["docs_single"] == 1 and st["docs_device"] == 0 and texts == ['{"m":{"a":3}}'], st

    monkeypatch.setenv("YCRDT_DOCS_CACHE", "0")
    texts, st = ask([d, pend])
    assert st["docs_single"] == 2 and st["docs_device"] == 0 and st["roots"] == 0 and texts == ['{"m":{"a":1}}', '{"m":{"a":2}}'], st
    monkeypatch.delenv("YCRDT_DOCS_CACHE")
    texts, st = ask([d])
    assert st["docs_single"] == 0 and st["docs_device"] == 1 and st["roots"] == 1 and texts == ['{"m":{"a":1}}'], st


def test_several_device_passes(monkeypatch):
    cs = [c for c in fixture_cases() if c["index"] == "ix" and c["name"] not in ("name_65", "empty")][:10]
    docs = [doc_of(*fixture_updates(c)) for c in cs]
    kw = dict(undefined={k: _undefined_names(c) for k, c in enumerate(cs)}, want={k: c["c"] for k, c in enumerate(cs)})
    one, st1 = ask(docs, **kw)
    assert st1["docs_device"] == len(docs), st1
    monkeypatch.setenv("YCRDT_DOCS_CACHE_PASS_BYTES", "600")
    many, st = ask(docs, **kw)
    assert many == one and st["docs_device"] == len(docs) and st["roots"] == st1["roots"], st
    monkeypatch.setenv("YCRDT_DOCS_CACHE_PASS_BYTES", "1")  # one document per pass
    many, st = ask(docs, **kw)
    assert many == one and st["docs_device"] == len(docs) and st["roots"] == st1["roots"], st


def test_no_document_and_argument_errors():
    import ctypes

    texts, st = crdt_amd.docs_cache_stats([])
    assert texts == [] and st["out_bytes"] == 0 and st["docs_device"] == st["docs_single"] == st["docs_empty"] == st["roots"] == 0
    d = _small()
    other = crdt_amd.Engine()
    with pytest.raises(crdt_amd.YcrdtError):
        crdt_amd.docs_cache([d], engine=other)  # a document of another engine
    L = crdt_amd.lib()
    hs = (ctypes.c_void_p * 1)(d._h.value)
    out, offs = crdt_amd._Out(), (ctypes.c_uint64 * 2)()
    assert L.ycrdt_docs_cache(d.engine._h, None, 1, b"ix", ctypes.byref(out), offs, None) == -6  # YCRDT_E_ARG
    assert L.ycrdt_docs_cache(d.engine._h, hs, 1, b"ix", None, offs, None) == -6
    assert L.ycrdt_docs_cache(d.engine._h, hs, 1, b"ix", ctypes.byref(out), None, None) == -6
    assert L.ycrdt_docs_cache(None, hs, 1, b"ix", ctypes.byref(out), offs, None) == -6
    assert not out.ptr and out.len == 0
    assert crdt_amd.docs_cache([d], index=None) == crdt_amd.docs_cache([d]) == ['{"m":{"a":1}}']  # a null index is "ix"


def test_other_fleet_calls_keep_their_path():
    """docs_json and docs_read share the front half and the placement kernels with the cache pass:
    over the same fleet, before and after a cache call, they answer on the device as they did."""
    cs = [c for c in fixture_cases() if c["name"] in ("basic", "array_per_key", "nested_levels", "values_0")]
    docs = [doc_of(*fixture_updates(c)) for c in cs]
    reqs = [(d, n, "array" if isinstance(v, list) else "map") for c, d in zip(cs, docs) for n, v in c["c"].items()]
    reads = [("map_size" if k == "map" else "array_length", d, n) for d, n, k in reqs] + [("map_get", docs[0], "users", "alice")]
    for _ in range(2):
        texts, st = crdt_amd.docs_json_stats([d for d, _, _ in reqs], [n for _, n, _ in reqs], [k for _, _, k in reqs])
        assert st["pairs_device"] == len(reqs) and st["pairs_single"] == 0, st
        assert texts == [d.root_json(n, k) for d, n, k in reqs]
        answers, rs = crdt_amd.docs_read_stats(reads)
        assert rs["reads_device"] == len(reads) and rs["reads_single"] == 0, rs
        assert answers[-1] == docs[0].map_get("users", "alice")
        _, cst = ask(docs, want={k: c["c"] for k, c in enumerate(cs)})
        assert cst["docs_device"] == len(docs), cst
