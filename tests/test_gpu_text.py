"""Text content on the device against Yjs 13.5.16 (tests/golden/text.json through tests/text_fixture.py):
concurrent Y.Text histories and hand-built ContentString updates, 31 of the 65 cases with a cut
between the two units of a surrogate pair. Yjs SPLITS a string there (an origin, a delete-set range, a
partly known duplicate, mergeUpdates' sliceStruct) and leaves U+FFFD on both sides for good; where it
WRITES at such an offset (encodeStateAsUpdate(doc, sv), diffUpdate) lib0 throws, and so does the
engine (YcrdtError). The mechanism is crdt_amd/csrc/yc_str.h (tests/test_str_piece.py holds it on the
host); here every entry point is held to the fixture: the state after one apply per update, after one
batch, in 13.5 order and in reversed order, the sync replies one by one and as one docs_diff call, the
doc-less update store, and the reads one by one and as one docs_json / docs_read call.

What is left out, and why:

    case            what      reason
    --------------  --------  -------------------------------------------------------------------
    map_empty       all       an empty ContentString item: Yjs keeps a struct of length 0, the
                              engine's unit tables have no place for a struct without units
    map_pair_last   json_m    Yjs reads a map entry's string value as its last UTF-16 unit
                              ("\\ude00"); the engine reads the last character, as its list reads give
                              one element per character

For the same reason list reads are compared after joining an adjacent (high, low) surrogate pair of
Yjs's per-unit elements into one element (join_pairs): in the fixture every lone surrogate of a
`json_t` is one of such a pair.
"""
import json

import pytest

crdt_amd = pytest.importorskip("crdt_amd")
from tests.text_fixture import all_cases, load  # noqa: E402
from tests.v1util import canonical_sv, canonical_update  # noqa: E402

pytestmark = pytest.mark.gpu

ME = 0x7FFFFFF0
EXCLUDED = {"map_empty": "all", "map_pair_last": "json_m"}  # (the table above)


def cases():
    return [c for c in all_cases() if EXCLUDED.get(c["name"]) != "all"]


def _high(x):
    return isinstance(x, str) and len(x) == 1 and 0xD800 <= ord(x) < 0xDC00


def _low(x):
    return isinstance(x, str) and len(x) == 1 and 0xDC00 <= ord(x) < 0xE000


def join_pairs(xs):
    out = []
    for x in xs:
        if _low(x) and out and _high(out[-1]):
            out[-1] = (out[-1] + x).encode("utf-16-le", "surrogatepass").decode("utf-16-le")
        else:
            out.append(x)
    assert not any(_high(x) or _low(x) for x in out)
    return out


def _doc(c, engine=None, order=1):
    d = crdt_amd.Doc(client_id=ME, engine=engine)
    for u in c["updates"][::order]:
        d.apply_update(u)
    return d


@pytest.fixture(scope="module")
def docs():
    """Every case as a document, one apply_update per update in the fixture's order."""
    cs = cases()
    return cs, [_doc(c) for c in cs]


@pytest.fixture(scope="module")
def e135():
    e = crdt_amd.Engine(compat=135)
    yield e
    e.close()


def test_cases_covered():
    assert len(all_cases()) == 65 and len(cases()) == 64
    assert sum(c["pair_split"] for c in cases()) >= 30
    assert len(load()["hand"]) == 16


# ---------------------------------------------------------------- state
def test_state_one_update_at_a_time(docs):
    for c, d in zip(*docs):
        assert d.encode_state_as_update() == c["state"], c["name"]
        assert canonical_sv(d.encode_state_vector()) == c["sv"], c["name"]
        assert d.pending() == (False, False), c["name"]


def test_state_one_batch():
    for c in cases():
        d = crdt_amd.Doc(client_id=ME)
        d.apply_updates(c["updates"])
        assert d.encode_state_as_update() == c["state"], c["name"]
        assert canonical_sv(d.encode_state_vector()) == c["sv"], c["name"]
        assert d.pending() == (False, False), c["name"]


def test_state_yjs_135_order(e135):
    for c in cases():
        d = _doc(c, e135)
        assert d.encode_state_as_update() == c["state_raw"], c["name"]
        assert d.pending() == (False, False), c["name"]


def test_state_reversed_order():
    fx = load()
    for c in fx["histories"] + [fx["long"]]:  # (the hand-built cases may depend on the order)
        d = _doc(c, order=-1)
        assert d.encode_state_as_update() == c["state_rev"], c["name"]
        assert d.pending() == (False, False), c["name"]


# ---------------------------------------------------------------- sync replies
def test_replies_one_by_one(docs):
    thrown = 0
    for c, d in zip(*docs):
        for r in c["replies"]:
            if r["update"] is None:
                with pytest.raises(crdt_amd.YcrdtError) as ei:
                    d.encode_state_as_update(r["sv"])
                assert ei.value.kind == "UNSUPPORTED" and "Yjs throws at this offset" in str(ei.value), (c["name"], str(ei.value))
                thrown += 1
            else:
                assert d.encode_state_as_update(r["sv"]) == r["update"], (c["name"], r["sv"].hex())
        assert d.encode_state_as_update() == c["state"], c["name"]  # a refusal leaves the document as it was
    assert thrown == 7


def test_replies_one_call(docs):
    pairs = [(c, d, r) for c, d in zip(*docs) for r in c["replies"]]
    good = [p for p in pairs if p[2]["update"] is not None]
    got = crdt_amd.docs_diff([d for _, d, _ in good], [r["sv"] for _, _, r in good])
    for (c, _, r), g in zip(good, got):
        assert g == r["update"], (c["name"], r["sv"].hex())
    for c, d, r in pairs:
        if r["update"] is None:
            with pytest.raises(crdt_amd.YcrdtError):
                crdt_amd.docs_diff([d], [r["sv"]])


# ---------------------------------------------------------------- the doc-less update store
def test_merge_updates():
    for c in cases():
        assert canonical_update(crdt_amd.merge_updates(c["updates"])) == c["merged"], c["name"]
        assert canonical_update(crdt_amd.merge_updates(c["updates"][::-1])) == c["merged_rev"], c["name"]


def test_merge_update_groups_one_call():
    cs = cases()
    got = crdt_amd.merge_update_groups([c["updates"] for c in cs] + [c["updates"][::-1] for c in cs])
    for c, g, gr in zip(cs, got[:len(cs)], got[len(cs):]):
        assert canonical_update(g) == c["merged"], c["name"]
        assert canonical_update(gr) == c["merged_rev"], c["name"]


def test_diff_update():
    thrown = 0
    good = []
    for c in cases():
        for r in c["replies"]:
            if r["diff"] is None:
                with pytest.raises(crdt_amd.YcrdtError) as ei:
                    crdt_amd.diff_update(c["merged"], r["sv"])
                assert ei.value.kind == "UNSUPPORTED" and "Yjs throws at this offset" in str(ei.value), (c["name"], str(ei.value))
                thrown += 1
            else:
                assert canonical_update(crdt_amd.diff_update(c["merged"], r["sv"])) == r["diff"], (c["name"], r["sv"].hex())
                good.append((c, r))
    assert thrown == 11
    got = crdt_amd.diff_updates([c["merged"] for c, _ in good], [r["sv"] for _, r in good])
    for (c, r), g in zip(good, got):
        assert canonical_update(g) == r["diff"], (c["name"], r["sv"].hex())


def test_state_vectors_from_updates():
    cs = cases()
    got = crdt_amd.state_vectors_from_updates([u for c in cs for u in c["updates"]])
    want = [sv for c in cs for sv in c["update_svs"]]
    tags = [(c["name"], i) for c in cs for i in range(len(c["updates"]))]
    for t, g, w in zip(tags, got, want):
        assert g == w, t


# ---------------------------------------------------------------- reads
def _want_m(c):
    return None if EXCLUDED.get(c["name"]) == "json_m" else json.loads(c["json_m"])


def _picks(n):
    return sorted({0, n // 2, n - 1}) if n else []


def test_reads_one_by_one(docs):
    for c, d in zip(*docs):
        if _want_m(c) is not None:
            assert json.loads(d.root_json("m", "map")) == _want_m(c), c["name"]
        want = join_pairs(json.loads(c["json_t"]))
        assert json.loads(d.root_json("t", "array")) == want, c["name"]
        assert d.array_length("t") == c["len_t"], c["name"]
        if len(want) == c["len_t"]:  # (no whole pair in the list: an index is a unit and an element)
            for i in _picks(len(want)):
                st, text = d.array_get("t", i)
                assert st == 1 and json.loads(text) == want[i], (c["name"], i)


def test_reads_one_call(docs):
    cs, ds = docs
    texts = crdt_amd.docs_json(ds + ds, ["m"] * len(ds) + ["t"] * len(ds), ["map"] * len(ds) + ["array"] * len(ds))
    for c, d, tm, tt in zip(cs, ds, texts[:len(ds)], texts[len(ds):]):
        if _want_m(c) is not None:
            assert json.loads(tm) == _want_m(c), c["name"]
        assert json.loads(tt) == join_pairs(json.loads(c["json_t"])), c["name"]
        assert (tm, tt) == (d.root_json("m", "map"), d.root_json("t", "array")), c["name"]
    reads, wants = [], []
    for c, d in zip(cs, ds):
        want = join_pairs(json.loads(c["json_t"]))
        reads.append(("array_length", d, "t"))
        wants.append((c["name"], c["len_t"]))
        if len(want) == c["len_t"]:
            for i in _picks(len(want)):
                reads.append(("array_get", d, "t", i))
                wants.append((c["name"], want[i]))
    for (name, w), g in zip(wants, crdt_amd.docs_read(reads)):
        if isinstance(g, tuple):
            assert g[0] == 1 and json.loads(g[1]) == w, (name, g)
        else:
            assert g == w, name


def test_docs_cache_nested(docs):
    """The text under `m.doc`: the cache refresh walks these documents without failing."""
    ds = [d for c, d in zip(*docs) if c.get("nested")]
    assert len(ds) >= 10
    for index in ("ix", "m"):
        assert len(crdt_amd.docs_cache(ds, index)) == len(ds)
