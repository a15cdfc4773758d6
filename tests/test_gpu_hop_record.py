"""Key resolution's 8-byte hop record (yc_work.h g_hop, yc_merge.hip seg_props_at / resolve_at).

A record holds the flags and ONE value word that is the list key (HOP_KEY) or the link up the
origin chain. k_resolve's climbers read, publish into and path-halve these records concurrently,
so the cases are the smallest histories at which a record can go wrong: chains that span several
workgroups of 256 segments (publishing and halving race across workgroups), one record read by
hundreds of climbers, a chain that ends in GC (a halving store may land over the GC conversion),
and a YArray chain (the list kind travels in the value word). Every case is compared byte for
byte, update and state vector, with the oracle port; it runs on the single-workgroup path and on
the grid kernels (YCRDT_MERGE_SMALL=0), three merges each of the forward and the reversed update
order in one process: a race shows up as a run that differs.
"""
import pytest

crdt_amd = pytest.importorskip("crdt_amd")

pytestmark = pytest.mark.gpu

PATHS = ["default", "grid"]


@pytest.fixture(params=PATHS)
def path(request, monkeypatch):
    if request.param == "grid":
        monkeypatch.setenv("YCRDT_MERGE_SMALL", "0")  # read when the batch is staged (merge_small_fits)
    else:
        monkeypatch.delenv("YCRDT_MERGE_SMALL", raising=False)
    return request.param


@pytest.fixture
def collide(monkeypatch):
    monkeypatch.setenv("YCRDT_KEY_HASH_BITS", "4")  # read when the batch is staged: every list in <= 16 hash values
    yield


def _any_int(v):  # lib0 `any` of a small integer (tag 125, signed varint)
    return bytes([125, v % 64])


def _varuint(v):
    out = bytearray()
    while v > 0x7F:
        out.append(0x80 | (v & 0x7F))
        v >>= 7
    out.append(v)
    return bytes(out)


def _delta(doc, sv_before):
    """What the replica wrote since sv_before: one struct per operation, never merged with the one
    before it (the encoder cuts at the state vector), so every operation is a segment of its own."""
    return doc.encode_state_as_update(sv_before)


def _reference(ups):
    from oracle.yref import Doc as ODoc

    ref = ODoc(0x7FFFFFF0)
    for u in ups:
        ref.apply_update(u)
    return ref.encode_state_as_update(), ref.encode_state_vector()


def _deep_chain(seed):
    """A base client sets 3 keys; replica A overwrites one of them 600 times (a chain over three
    workgroups), replica B the same key 300 times, concurrently."""
    from oracle.yref import Doc as ODoc

    base = ODoc(1)
    for k in range(3):
        base.map_set("users", f"key{k}", _any_int(seed + k))
    b = base.encode_state_as_update()
    ups = [b]
    for client, n in ((100, 600), (200, 300)):
        d = ODoc(client)
        d.apply_update(b)
        for i in range(n):
            sv = d.encode_state_vector()
            d.map_set("users", "key1", _any_int(seed + client + i))
            ups.append(_delta(d, sv))
    return ups


def _wide_fan(seed):
    """One root item with one child each from 700 clients."""
    from oracle.yref import Doc as ODoc

    base = ODoc(1)
    base.map_set("users", "key0", _any_int(seed))
    b = base.encode_state_as_update()
    ups = [b]
    for r in range(700):
        d = ODoc(100 + r)
        d.apply_update(b)
        sv = d.encode_state_vector()
        d.map_set("users", "key0", _any_int(seed + r))
        ups.append(_delta(d, sv))
    return ups


def _gc_chain():
    """A GC struct of client 5, then 300 items of client 9, each with origin = the one before it and
    the first with origin = the GC unit; one update per item (Yjs v1 bytes: info 0x88 = origin |
    ContentAny, the origin id, one `any`), so none arrives merged."""
    ups = [_varuint(1) + _varuint(1) + _varuint(5) + _varuint(0) + bytes([0]) + _varuint(1) + _varuint(0)]
    for i in range(300):
        origin = (5, 0) if i == 0 else (9, i - 1)
        item = bytes([0x88]) + _varuint(origin[0]) + _varuint(origin[1]) + _varuint(1) + _any_int(i)
        ups.append(_varuint(1) + _varuint(1) + _varuint(9) + _varuint(i) + item + _varuint(0))
    return ups


def _array_chain():
    """600 single pushes by one client, no parentSub: a YArray chain 600 deep."""
    from oracle.yref import Doc as ODoc

    d = ODoc(100)
    ups = []
    for i in range(600):
        sv = d.encode_state_vector()
        d.array_insert("list", i, [_any_int(i)])
        ups.append(_delta(d, sv))
    return ups


_CASES = {"deep_chain": lambda: _deep_chain(0), "wide_fan": lambda: _wide_fan(0), "gc_chain": _gc_chain, "array_chain": _array_chain}
_cache = {}


def _case(name):
    """(updates, oracle update, oracle state vector), built once per session and never changed."""
    if name not in _cache:
        ups = _CASES[name]()
        _cache[name] = (ups,) + _reference(ups)
    return _cache[name]


def _docs_case():
    """The deep chain and the wide fan as three documents each, the same key names in all six."""
    if "docs" not in _cache:
        docs = [_deep_chain(7 * i + 1) for i in range(3)] + [_wide_fan(5 * i + 2) for i in range(3)]
        _cache["docs"] = (docs, [_reference(ups) for ups in docs])
    return _cache["docs"]


def _merge_single(ups, want_u, want_sv):
    for order in (ups, ups[::-1]):
        for rep in range(3):
            b = crdt_amd.Batch(order)
            b.merge()
            u, sv = b.result()
            assert u == want_u, (len(order), rep, order is ups)
            assert sv == want_sv, (len(order), rep, order is ups)


def _merge_docs(docs, want):
    for fwd in (True, False):
        staged = docs if fwd else [ups[::-1] for ups in docs]
        for rep in range(3):
            b = crdt_amd.Batch(docs=staged)
            b.merge()
            assert b.result_docs() == want, (rep, fwd)


@pytest.mark.parametrize("name", sorted(_CASES))
def test_hop_record_case(name, path):
    ups, want_u, want_sv = _case(name)
    _merge_single(ups, want_u, want_sv)


@pytest.mark.parametrize("name", ["deep_chain", "wide_fan"])
def test_hop_record_case_collisions(name, path, collide):
    ups, want_u, want_sv = _case(name)
    _merge_single(ups, want_u, want_sv)


def test_hop_record_shapes():
    """The histories are what the cases need: the chain case's winner is replica B's last write
    (the max-client descent's leaf), the GC chain turns every item into GC, the array keeps order."""
    import json

    from oracle.yref import Doc as ODoc

    ref = ODoc(0x7FFFFFF0)
    ref.apply_update(_case("deep_chain")[1])
    assert json.loads(ref.root_json("users", "map"))["key1"] == (200 + 299) % 64
    ref = ODoc(0x7FFFFFF0)
    ref.apply_update(_case("wide_fan")[1])
    assert json.loads(ref.root_json("users", "map"))["key0"] == 699 % 64
    # client 9: one GC run of 300 (info 0, length 300), client 5: the GC struct; both in the delete set
    structs = _varuint(2) + _varuint(1) + _varuint(9) + _varuint(0) + bytes([0]) + _varuint(300) + _varuint(1) + _varuint(5) + _varuint(0) + bytes([0]) + _varuint(1)
    ds = _varuint(2) + _varuint(9) + _varuint(1) + _varuint(0) + _varuint(300) + _varuint(5) + _varuint(1) + _varuint(0) + _varuint(1)
    assert _case("gc_chain")[1] == structs + ds
    ref = ODoc(0x7FFFFFF0)
    ref.apply_update(_case("array_chain")[1])
    assert json.loads(ref.root_json("list", "array")) == [i % 64 for i in range(600)]


def test_hop_record_multidoc(path):
    docs, refs = _docs_case()
    _merge_docs(docs, refs)


def test_hop_record_multidoc_collisions(path, collide):
    docs, refs = _docs_case()
    _merge_docs(docs, refs)
