"""The encode record (yc_encrec.h; yc_encode.hip out_sizes_at -> k_write_structs), the per-client
output base (CC64_OUTBASE / CC_OPOS0) and the first output struct of every client taken from the
size pass (CC_FIRST_OUT).

Every case is compared byte for byte, update and state vector, with the oracle port, and between
YCRDT_ENC_RECORD unset and =0 (no valid record: every struct is encoded from its columns, as before
the record existed). Every case runs on the default path (the single-workgroup kernels) and on the
grid kernels (YCRDT_MERGE_SMALL=0 YCRDT_ENCODE_SMALL=0), with the forward and the reversed update
order. The cases are the smallest at which the record, its 11-bit widths or the per-client words can
go wrong: client boundaries inside a workgroup, header lengths / content lengths / deleted lengths
of 2040..2056 (2047 is the last a record holds), structs with and without a record side by side in
one wavefront, a delta encode (no record, outputs of size 0), several documents, several byte
windows (no record), no struct at all and one struct.
"""
import pytest

crdt_amd = pytest.importorskip("crdt_amd")

pytestmark = pytest.mark.gpu

PATHS = ["default", "grid"]
EDGE = range(2040, 2057)  # 17 widths across the 11-bit limit


@pytest.fixture(params=PATHS)
def path(request, monkeypatch):
    for k in ("YCRDT_MERGE_SMALL", "YCRDT_ENCODE_SMALL", "YCRDT_ENC_RECORD", "YCRDT_WIN_SHIFT"):
        monkeypatch.delenv(k, raising=False)
    if request.param == "grid":
        monkeypatch.setenv("YCRDT_MERGE_SMALL", "0")  # read when the batch is staged
        monkeypatch.setenv("YCRDT_ENCODE_SMALL", "0")
    return request.param


def _any_int(v):  # lib0 `any` of a small integer (tag 125, signed varint)
    return bytes([125, v % 64])


def _varuint(v):
    out = bytearray()
    while v > 0x7F:
        out.append(0x80 | (v & 0x7F))
        v >>= 7
    out.append(v)
    return bytes(out)


def _varstr(s):
    b = s.encode()
    return _varuint(len(b)) + b


def _any_str(s):  # lib0 `any` of a string (tag 119)
    return bytes([119]) + _varstr(s)


def _one(client, clock, item):
    """An update of one struct and an empty delete set (Yjs v1 bytes)."""
    return _varuint(1) + _varuint(1) + _varuint(client) + _varuint(clock) + item + _varuint(0)


def _reference(ups, sv=b""):
    from oracle.yref import Doc as ODoc

    ref = ODoc(0x7FFFFFF0)
    for u in ups:
        ref.apply_update(u)
    return ref.encode_state_as_update(sv), ref.encode_state_vector()


def _boundary_mix(seed):
    """A base client sets 7 keys of YMap `users`; five replicas each overwrite them 130 times, one
    delta per operation: 657 structs in six client blocks, the boundaries inside workgroups."""
    from oracle.yref import Doc as ODoc

    base = ODoc(1)
    for k in range(7):
        base.map_set("users", f"key{k}", _any_int(seed + k))
    b = base.encode_state_as_update()
    ups = [b]
    for r in range(5):
        d = ODoc(100 + r)
        d.apply_update(b)
        for i in range(130):
            sv = d.encode_state_vector()
            d.map_set("users", f"key{(i + r) % 7}", _any_int(seed + 3 * r + i))
            ups.append(d.encode_state_as_update(sv))
    return ups


def _header_edges():
    """Root-level map entries: info, 1, "users", the key. Between the info byte and the content lie
    1 + 6 + 2 + len(key) bytes for a key of 128..16383 bytes: 2040..2056 for keys of 2031..2047."""
    from oracle.yref import Doc as ODoc

    d = ODoc(7)
    ups = []
    for h in EDGE:
        sv = d.encode_state_vector()
        d.map_set("users", "k" * (h - 9 - 5) + f"{h:05d}", _any_int(h))
        ups.append(d.encode_state_as_update(sv))
    return ups


def _content_edges():
    """String values: the content (element count, tag 119, two length bytes, the text) is
    4 + len(text) bytes: 2040..2056 for texts of 2036..2052 bytes."""
    from oracle.yref import Doc as ODoc

    d = ODoc(7)
    ups = []
    for n in EDGE:
        sv = d.encode_state_vector()
        d.map_set("users", f"k{n}", _any_str("v" * (n - 4)))
        ups.append(d.encode_state_as_update(sv))
    return ups


def _deleted_edges():
    """One ContentDeleted item of length 2040..2056 each, under the root array `list` (info 1 =
    ContentDeleted without origins, parent by name, the length), every one from a client of its own."""
    return [_one(300 + k, 0, bytes([1]) + _varuint(1) + _varstr("list") + _varuint(n)) for k, n in enumerate(EDGE)]


def _deferred_beside_fast():
    """Client 50 pushes 150 multi-character strings to the root array `list`, every second one as a
    ContentString (one unit per character), the others as a ContentAny holding the string (one unit),
    so that no two neighbours merge; client 60 inserts an item into the middle of every ContentString.
    Each of those is split in two and goes to the general encoder, the others and client 60's items
    are whole: structs with and without a record alternate."""
    ups = []
    clock = 0
    splits = []
    for i in range(150):
        text = f"s{i:03d}"  # 4 characters
        if i % 2:
            content, ref, n = _varstr(text), 4, len(text)
        else:
            content, ref, n = _varuint(1) + _any_str(text), 8, 1
        if i == 0:
            item = bytes([ref]) + _varuint(1) + _varstr("list") + content
        else:
            item = bytes([0x80 | ref]) + _varuint(50) + _varuint(clock - 1) + content
        ups.append(_one(50, clock, item))
        if i % 2:
            splits.append(clock + 1)  # between the second and the third character
        clock += n
    for j, c in enumerate(splits):
        item = bytes([0xC8]) + _varuint(50) + _varuint(c) + _varuint(50) + _varuint(c + 1) + _varuint(1) + _any_int(j)
        ups.append(_one(60, j, item))
    return ups


def _empty():
    return [_varuint(0) + _varuint(0)]


def _one_struct():
    from oracle.yref import Doc as ODoc

    d = ODoc(5)
    d.map_set("users", "key0", _any_int(1))
    return [d.encode_state_as_update()]


_CASES = {
    "boundary_mix": lambda: _boundary_mix(0),
    "header_edges": _header_edges,
    "content_edges": _content_edges,
    "deleted_edges": _deleted_edges,
    "deferred_beside_fast": _deferred_beside_fast,
    "empty": _empty,
    "one_struct": _one_struct,
}
_cache = {}


def _case(name):
    """(updates, oracle update, oracle state vector), built once per session and never changed."""
    if name not in _cache:
        ups = _CASES[name]()
        _cache[name] = (ups,) + _reference(ups)
    return _cache[name]


def _docs_case():
    if "docs" not in _cache:
        docs = [_boundary_mix(11 * i + 1) for i in range(3)]
        _cache["docs"] = (docs, [_reference(ups) for ups in docs])
    return _cache["docs"]


def _both_settings(monkeypatch, run):
    """run() with YCRDT_ENC_RECORD unset and =0 (read when the batch is staged): (with records, without)."""
    monkeypatch.delenv("YCRDT_ENC_RECORD", raising=False)
    on = run()
    monkeypatch.setenv("YCRDT_ENC_RECORD", "0")
    off = run()
    monkeypatch.delenv("YCRDT_ENC_RECORD", raising=False)
    return on, off


def _merge(ups):
    b = crdt_amd.Batch(ups)
    b.merge()
    return b.result()


@pytest.mark.parametrize("name", sorted(_CASES))
def test_encode_record_case(name, path, monkeypatch):
    ups, want_u, want_sv = _case(name)
    for order in (ups, ups[::-1]):
        on, off = _both_settings(monkeypatch, lambda: _merge(order))
        assert on == (want_u, want_sv), (name, order is ups)
        assert off == (want_u, want_sv), (name, order is ups)
        assert on == off


def test_encode_record_shapes():
    """The histories are what the cases need: the widths straddle 2047 and the split case splits."""
    ups, want_u, _ = _case("header_edges")
    for h, u in zip(EDGE, ups):  # client block header 1 1 7 clock, then info | header | content (3 bytes)
        body = u[2 + len(_varuint(7)) + len(_varuint(h - 2040)):-1]
        assert len(body) == 1 + h + 3 and body[0] == 0x28, h
    ups, _, _ = _case("content_edges")
    for n, u in zip(EDGE, ups):
        assert u.count(b"v" * (n - 4)) == 1 and bytes([1, 119]) + _varuint(n - 4) in u, n
    _, want_u, _ = _case("deleted_edges")
    for n in EDGE:
        assert bytes([1, 1]) + _varstr("list") + _varuint(n) in want_u, n
    # 75 ContentStrings in two halves each (the second half: origin | ContentString, two characters)
    ups, want_u, _ = _case("deferred_beside_fast")
    assert len(ups) == 225
    for i in range(1, 150, 2):
        text = f"s{i:03d}"
        assert _varstr(text[:2]) in want_u and _varstr(text[2:]) in want_u and _varstr(text) not in want_u, i
    assert _case("empty")[1] == bytes([0, 0])


def test_encode_record_delta(path, monkeypatch):
    """A delta encode against a state vector that cuts two clients mid-way (one of them inside a
    struct's client block, every struct of length 1): the whole-item encoder declines, outputs below
    the target have size 0 and write nothing."""
    ups, _, _ = _case("boundary_mix")
    # client 1 known whole, 100 and 102 cut mid-way, 101 known whole, 103 / 104 unknown
    sv = _varuint(4) + b"".join(_varuint(c) + _varuint(k) for c, k in ((1, 7), (100, 65), (101, 130), (102, 40)))
    want_u, want_sv = _reference(ups, sv)
    assert 100 < len(want_u) < len(_case("boundary_mix")[1])

    def run():
        d = crdt_amd.Doc(client_id=0x7FFFFFF0)
        d.apply_updates(order)
        return d.encode_state_as_update(sv), d.encode_state_vector(), d.encode_state_as_update()

    for order in (ups, ups[::-1]):
        on, off = _both_settings(monkeypatch, run)
        assert on == (want_u, want_sv, _case("boundary_mix")[1]), order is ups
        assert on == off


def test_encode_record_multidoc(path, monkeypatch):
    """Three documents in one batch: each equals the document merged alone (and the oracle)."""
    docs, refs = _docs_case()
    alone = [_merge(ups) for ups in docs]
    assert alone == refs

    for fwd in (True, False):
        staged = docs if fwd else [ups[::-1] for ups in docs]

        def run():
            b = crdt_amd.Batch(docs=staged)
            b.merge()
            return b.result_docs()

        on, off = _both_settings(monkeypatch, run)
        assert on == alone, fwd
        assert on == off


def test_encode_record_windows(path, monkeypatch):
    """The three-document batch in byte windows of 64 KiB: a record holds a position within one
    window, so none is valid in a batch of several, and the bytes are those of the one-window merge."""
    docs, refs = _docs_case()
    assert sum((len(u) + 63) // 64 * 64 for ups in docs for u in ups) > (1 << 16), "the batch must span several windows"
    monkeypatch.setenv("YCRDT_WIN_SHIFT", "16")

    for fwd in (True, False):
        staged = docs if fwd else [ups[::-1] for ups in docs]

        def run():
            b = crdt_amd.Batch(docs=staged)
            b.merge()
            return b.result_docs()

        on, off = _both_settings(monkeypatch, run)
        assert on == refs, fwd
        assert on == off
