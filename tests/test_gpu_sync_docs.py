"""Sync replies for many (document, peer state vector) pairs in one device pass (ycrdt_docs_diff,
yc_sync.hip): every reply against the real Yjs (tests/golden/sync.json, configs.json) and against
the per-doc path it must equal byte for byte; the stats prove which path answered."""
import random

import pytest

crdt_amd = pytest.importorskip("crdt_amd")

from oracle.yref import Doc as ODoc  # noqa: E402
from tests.sync_util import blocks, load_cases  # noqa: E402
from tests.v1util import canonical_update  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [c for c in load_cases("sync") if c["name"] != "text_pair_inside"]


def _vu(v):
    out = bytearray()
    while v > 127:
        out.append(0x80 | (v & 0x7F))
        v >>= 7
    out.append(v)
    return bytes(out)


def _sv(entries):
    return _vu(len(entries)) + b"".join(_vu(c) + _vu(k) for c, k in entries)


def _marked_doc(updates, engine=None):
    """A doc merged on its own (one flush): its state carries the encoder's marks."""
    d = crdt_amd.Doc(client_id=0x7FFFFFF0, engine=engine)
    d.apply_updates(list(updates))
    d.flush()
    return d


def _fleet(update_lists):
    """Docs merged together by apply_updates_multi: their states carry no marks."""
    assert len(update_lists) >= 2
    docs = [crdt_amd.Doc(client_id=0x7FFFFFF0) for _ in update_lists]
    pairs = [(i, u) for i, ups in enumerate(update_lists) for u in ups]
    crdt_amd.apply_updates_multi([docs[i] for i, _ in pairs], [u for _, u in pairs])
    return docs


def _fixture_pairs(docs):
    """(doc, sv, Yjs's reply) of every recorded pair of the sync fixture."""
    out = []
    for d, c in zip(docs, CASES):
        for r in c["replies"]:
            out.append((d, bytes.fromhex(r["sv"]), bytes.fromhex(r["update"])))
    return out


def _check_pairs(pairs, **want):
    got, st = crdt_amd.docs_diff_stats([p[0] for p in pairs], [p[1] for p in pairs])
    assert len(got) == len(pairs)
    for (d, sv, ref), g in zip(pairs, got):
        if ref is not None:
            assert canonical_update(g).hex() == ref.hex(), sv.hex()
        assert g.hex() == d.encode_state_as_update(sv).hex(), sv.hex()
    for k, v in want.items():
        assert st[k] == v, (k, st)
    assert st["out_bytes"] == sum(len(g) for g in got)
    return st


def test_fixture_cases_from_marks():
    docs = [_marked_doc([bytes.fromhex(u) for u in c["updates"]]) for c in CASES]
    pairs = _fixture_pairs(docs)
    st = _check_pairs(pairs, pairs_marks=len(pairs), pairs_walk=0, pairs_single=0)
    assert st["cut_structs"] > 0
    random.Random(7).shuffle(pairs)
    st2 = _check_pairs(pairs, pairs_marks=len(pairs), pairs_single=0)
    assert st2["cut_structs"] == st["cut_structs"]


def test_fixture_cases_walked():
    docs = _fleet([[bytes.fromhex(u) for u in c["updates"]] for c in CASES])
    pairs = _fixture_pairs(docs)
    st = _check_pairs(pairs, pairs_walk=len(pairs), pairs_marks=0, pairs_single=0)
    assert st["cut_structs"] > 0
    random.Random(8).shuffle(pairs)
    _check_pairs(pairs, pairs_walk=len(pairs), pairs_single=0)


def test_cut_inside_a_surrogate_pair_is_the_single_path():
    """Yjs 13.5.16 throws on this cut; the slice helper refuses it and the pair gets what the
    per-doc path gives: the same error."""
    c = next(c for c in load_cases("sync") if c["name"] == "text_pair_inside")
    d = _marked_doc([bytes.fromhex(u) for u in c["updates"]])
    sv = bytes.fromhex(c["replies"][0]["sv"])
    with pytest.raises(crdt_amd.YcrdtError) as single:
        d.encode_state_as_update(sv)
    with pytest.raises(crdt_amd.YcrdtError) as batched:
        crdt_amd.docs_diff([d, d], [b"", sv])
    assert batched.value.code == single.value.code
    assert crdt_amd.docs_diff([d], [b""])[0] == d.encode_state_as_update()


def test_recorded_pairs_of_configs():
    cases = [c for c in load_cases("configs") if c["name"][:3] in ("c3_", "c4_", "c5_")]
    ups = [[bytes.fromhex(u) for u in c["updates"]] for c in cases]
    docs = [None] * len(cases)
    odd = [i for i in range(len(cases)) if i % 2]
    for i, d in zip(odd, _fleet([ups[i] for i in odd])):
        docs[i] = d
    for i in range(0, len(cases), 2):
        docs[i] = _marked_doc(ups[i])
    pairs, nmarks, nsingle = [], 0, 0
    walk_max = crdt_amd.docs_diff_stats([], [])[1]["walk_max"]
    for i, (d, c) in enumerate(zip(docs, cases)):
        mine = [(d, b"", bytes.fromhex(c["state"])), (d, b"\x00", bytes.fromhex(c["state"]))]
        mine += [(d, bytes.fromhex(r["sv"]), bytes.fromhex(r["update"])) for r in c["diffs"]]
        pairs += mine
        if i % 2 == 0:
            nmarks += len(mine)
        elif len(c["state"]) // 2 > walk_max:
            nsingle += len(mine)
    assert len(pairs) >= 180 + 2 * len(cases)
    _check_pairs(pairs, pairs_marks=nmarks, pairs_single=nsingle, pairs_walk=len(pairs) - nmarks - nsingle)


def _any_int(v):
    return bytes([125, v])  # lib0 any: a small varint


@pytest.fixture(scope="module")
def big_doc_updates():
    """Three clients: 1 000 single-value structs (a block of many bitmap words), pushes that merge
    into long ContentAny structs with deleted runs cut out, and a map with overwritten keys."""
    a, b, c = ODoc(1001), ODoc(1002), ODoc(0x30000003)
    for i in range(1000):
        a.array_insert("a", 0, [_any_int(i % 60)])
    for i in range(40):
        b.array_insert("b", 10 * i, [_any_int(j) for j in range(10)])
    b.array_delete("b", 35, 90)
    b.array_delete("b", 200, 3)
    for i in range(120):
        c.map_set("m", f"key{i % 7}", _any_int(i % 50))
    return [x.encode_state_as_update() for x in (a, b, c)]


def test_one_doc_many_peers(big_doc_updates):
    d = _marked_doc(big_doc_updates)
    ends = {b["client"]: b["end_clock"] for b in blocks(d.encode_state_as_update())[0]}
    assert max(b["end"] - b["first"] for b in blocks(d.encode_state_as_update())[0]) > 64 * 64  # (more bitmap words than one wave step)
    rng = random.Random(20261019)
    svs = []
    for _ in range(200):
        svs.append(_sv([(c, rng.randint(0, e)) for c, e in sorted(ends.items(), key=lambda kv: rng.random())]))
    st = _check_pairs([(d, sv, None) for sv in svs], pairs_marks=200, pairs_single=0)
    assert st["cut_structs"] > 100  # (client 1002's few long structs: nearly every clock cuts one)
    # the same document without marks
    w = _fleet([big_doc_updates, big_doc_updates[:1]])[0]
    _check_pairs([(w, sv, None) for sv in svs[:50]], pairs_walk=50, pairs_single=0)


def test_cut_around_a_wave_step():
    """The search takes 64 bitmap words per wave step: cuts inside the structs that start in the
    last words of one step and the first of the next (and the struct that straddles them)."""
    a = ODoc(21)
    for i in range(500):
        a.array_insert("a", 0, [_any_int(i % 60), _any_int(1), _any_int(2)])
    d = _marked_doc([a.encode_state_as_update()])
    (b,), _ = blocks(d.encode_state_as_update())
    assert b["end"] - b["first"] > 64 * 64
    w0 = b["first"] >> 6
    near = [s for pos, s in b["structs"] if (pos >> 6) - w0 in (62, 63, 64, 65)]
    assert len(near) >= 8 and all(s.length == 3 for s in near)
    svs = [_sv([(21, s.clock + off)]) for s in near for off in (0, 1, 2)]
    st = _check_pairs([(d, sv, None) for sv in svs], pairs_marks=len(svs), pairs_single=0)
    assert st["cut_structs"] == 2 * len(near)
    w = _fleet([[a.encode_state_as_update()], [a.encode_state_as_update()]])[0]
    _check_pairs([(w, sv, None) for sv in svs], pairs_walk=len(svs), pairs_single=0)


@pytest.mark.parametrize("target", [63, 0, 1])
def test_block_start_at_a_bitmap_word_edge(target):
    """The second block's first struct at byte offset = 63 / 0 / 1 mod 64 (a key's length pads the
    first block): the first and last bitmap words of a block are masked at their edges."""
    lo = ODoc(5)
    lo.array_insert("a", 0, [_any_int(j) for j in range(6)])
    lo.array_insert("a", 0, [_any_int(9)])
    lo.array_insert("a", 3, [_any_int(8), _any_int(7)])
    found = None
    for pad in range(1, 200):
        hi = ODoc(6)
        hi.map_set("m", "k" * pad, _any_int(1))
        hi.array_insert("z", 0, [_any_int(j) for j in range(5)])
        ref = ODoc(0x7FFFFFF0)
        for u in (hi.encode_state_as_update(), lo.encode_state_as_update()):
            ref.apply_update(u)
        bl = blocks(ref.encode_state_as_update())[0]
        if bl[1]["client"] == 5 and bl[1]["first"] % 64 == target:
            found = [hi.encode_state_as_update(), lo.encode_state_as_update()]
            break
    assert found, "no padding puts the block there"
    svs = [_sv([(5, k), (6, j)]) for k in range(0, 10) for j in (0, 1, 3, 6)]
    d = _marked_doc(found)
    _check_pairs([(d, sv, None) for sv in svs], pairs_marks=len(svs), pairs_single=0)
    w = _fleet([found, found[:1]])[0]
    _check_pairs([(w, sv, None) for sv in svs], pairs_walk=len(svs), pairs_single=0)


def test_routing_to_the_single_path(big_doc_updates):
    # pending structs
    c = next(c for c in load_cases("pending") if c["name"] == "kat_gap")
    p = crdt_amd.Doc(client_id=0x7FFFFFF0)
    p.apply_update(bytes.fromhex(c["updates"][0]))
    assert any(p.pending())
    svs = [b"", b"\x00", bytes.fromhex(c["steps"][0]["sv"])]
    _check_pairs([(p, sv, None) for sv in svs], pairs_single=len(svs), pairs_marks=0, pairs_walk=0)
    # an empty doc: 00 00, whatever the peer says
    e = crdt_amd.Doc(client_id=3)
    got, st = crdt_amd.docs_diff_stats([e, e], [b"", _sv([(1, 4)])])
    assert got == [b"\x00\x00", b"\x00\x00"] and st["pairs_single"] == st["pairs_marks"] == st["pairs_walk"] == 0
    # a mark-less state larger than walk_max
    big = ODoc(77)
    for i in range(300):
        big.array_insert("a", 0, [bytes([119, 0xFF, 0x01]) + b"x" * 255])  # a 255-byte string each
    docs = _fleet([[big.encode_state_as_update()], big_doc_updates])
    walk_max = crdt_amd.docs_diff_stats([], [])[1]["walk_max"]
    assert len(docs[0].encode_state_as_update()) > walk_max > len(docs[1].encode_state_as_update())
    pairs = [(docs[0], _sv([(77, 150)]), None), (docs[1], _sv([(1001, 500)]), None), (docs[0], b"", None)]
    _check_pairs(pairs, pairs_single=2, pairs_walk=1, pairs_marks=0)


def test_routing_compat_135():
    import os

    e135 = crdt_amd.Engine(int(os.environ.get("YCRDT_DEVICE", "0")), compat=135)
    c = next(c for c in CASES if c["name"] == "big_clients")
    d = _marked_doc([bytes.fromhex(u) for u in c["updates"]], engine=e135)
    svs = [bytes.fromhex(r["sv"]) for r in c["replies"]]
    got, st = crdt_amd.docs_diff_stats([d] * len(svs), svs, engine=e135)
    assert [g.hex() for g in got] == [d.encode_state_as_update(sv).hex() for sv in svs]
    assert st["pairs_single"] == len(svs) and st["pairs_marks"] == 0


def test_switch_forces_the_single_path(monkeypatch):
    c = next(c for c in CASES if c["name"] == "wave_steps")
    d = _marked_doc([bytes.fromhex(u) for u in c["updates"]])
    pairs = [(d, bytes.fromhex(r["sv"]), bytes.fromhex(r["update"])) for r in c["replies"]]
    monkeypatch.setenv("YCRDT_SYNC", "0")
    _check_pairs(pairs, pairs_single=len(pairs), pairs_marks=0, pairs_walk=0)
    monkeypatch.delenv("YCRDT_SYNC")
    _check_pairs(pairs, pairs_single=0, pairs_marks=len(pairs))


def test_truncated_state_vector_fails_the_call_only():
    c = next(c for c in CASES if c["name"] == "push123")
    d = _marked_doc([bytes.fromhex(u) for u in c["updates"]])
    good = bytes.fromhex(c["replies"][0]["sv"])
    with pytest.raises(crdt_amd.YcrdtError) as ei:
        crdt_amd.docs_diff([d, d], [good, b"\x02\x03\x01"])
    assert ei.value.kind == "DECODE"
    _check_pairs([(d, good, bytes.fromhex(c["replies"][0]["update"]))], pairs_marks=1)


def test_state_vector_entry_orders():
    """Clients ascending, descending, in no order, and one named twice (its last clock counts, as in
    the per-doc path's map)."""
    c = next(c for c in CASES if c["name"] == "big_clients")
    d = _marked_doc([bytes.fromhex(u) for u in c["updates"]])
    a, b = 0x10000005, 0xF0000001
    svs = [_sv([(a, 2), (b, 1)]), _sv([(b, 1), (a, 2)]), _sv([(b, 1), (7, 9), (a, 2)]), _sv([(a, 1), (b, 1), (a, 2)]),
           _sv([(b, 3), (a, 2), (b, 1)])]
    got, st = crdt_amd.docs_diff_stats([d] * len(svs), svs)
    assert st["pairs_marks"] == len(svs)
    assert len(set(got)) == 1 and got[0] == d.encode_state_as_update(svs[0])
    for sv, g in zip(svs, got):
        assert g == d.encode_state_as_update(sv)


def test_marks_follow_the_state():
    """After a reply, one more update: the next reply is planned from the new state's marks."""
    c = next(c for c in CASES if c["name"] == "sv_edges")
    ups = [bytes.fromhex(u) for u in c["updates"]]
    d = _marked_doc(ups[:1])
    o = ODoc(0x7FFFFFF0)
    o.apply_update(ups[0])
    sv = _sv([(11, 1)])
    assert crdt_amd.docs_diff([d], [sv])[0] == o.encode_state_as_update(sv)
    d.apply_update(ups[1])
    o.apply_update(ups[1])
    for v in (sv, _sv([(12, 1), (11, 2)]), b""):
        got, st = crdt_amd.docs_diff_stats([d], [v])
        assert got[0] == o.encode_state_as_update(v) and st["pairs_marks"] == 1
    for r in c["replies"]:
        assert canonical_update(crdt_amd.docs_diff([d], [bytes.fromhex(r["sv"])])[0]).hex() == r["update"]
