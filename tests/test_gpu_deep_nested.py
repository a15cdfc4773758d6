"""Types nested up to six levels below a root, against Yjs 13.5.16 (tests/golden/deep.json,
tests/golden/gen/gen_deep_fixtures.js): types inside YArrays and inside nested types, deletes and
overwrites that kill whole subtrees, inserts into containers another replica had already deleted,
full states whose GC structs cover what other inputs carry as live items, a nested list with 300
concurrent roots, a parent that arrives as a GC struct, children that arrive before their parent.

That is the ground of yc_merge.hip's dead-ancestor climb (k_dead_init / k_dead_climb / k_dead_apply)
and of its k_parent / KF_PSUB writes, of yc_ingest.cpp's parent lookup, of the sharded and the
multi-document merge with a dead ancestor in another shard or beside other documents, of the level
rounds of docs_json and of docs_diff over states full of GC runs.

Every update is compared by the one rule of tests/deep_fixture.py: exact bytes wherever Yjs's own
bytes do not depend on its apply order, else after merging adjacent GC structs on both sides; state
vectors, toJSON, pending flags and delete sets exactly. tests/test_deep_fixture.py holds the share
of coalesced comparisons under a quarter and the oracle to Yjs's forward bytes.
"""
import json
import random

import pytest

crdt_amd = pytest.importorskip("crdt_amd")
from tests.deep_fixture import assert_same_update, coalesced, hand_built, load, quiet_cases, random_sample, sha  # noqa: E402
from tests.v1util import canonical_sv  # noqa: E402

pytestmark = pytest.mark.gpu

PARTS = 4
ME = 0x7FFFFFF0


@pytest.fixture(params=["default", "grid", "collide", "grid_collide"])
def path(request, monkeypatch):
    """The single-workgroup merge or the grid kernels, every list in its own hash value or all of
    them in 16 (both switches are read when the batch is staged)."""
    monkeypatch.delenv("YCRDT_MERGE_SMALL", raising=False)
    monkeypatch.delenv("YCRDT_KEY_HASH_BITS", raising=False)
    if "grid" in request.param:
        monkeypatch.setenv("YCRDT_MERGE_SMALL", "0")
    if "collide" in request.param:
        monkeypatch.setenv("YCRDT_KEY_HASH_BITS", "4")
    return request.param


def _sampled():
    """The hand-built cases and 15 random ones: what the merge-path and shard tests run."""
    return hand_built() + random_sample(15)


def _merge(ups, nshards=None):
    b = crdt_amd.Batch(ups)
    if nshards is None:
        b.merge()
    else:
        b.merge_sharded(nshards)
    return b.result()


_single = {}


def _single_state(c):
    """(state, state vector) of the case merged on its own, once per session."""
    if c["name"] not in _single:
        _single[c["name"]] = _merge(c["updates"])
    return _single[c["name"]]


# ---------------------------------------------------------------- one document
def _check_doc(d, c, tag):
    fx = load()
    assert d.pending() == c["pending"], tag
    assert_same_update(d.encode_state_as_update(), c["state"], tag)
    assert sha(canonical_sv(d.encode_state_vector())) == c["sv"], tag
    for k, r in enumerate(c["diffs"]):
        assert_same_update(d.encode_state_as_update(r["sv"]), r["update"], tag + (k,))
    for root, kind in fx["roots"].items():
        assert json.loads(d.root_json(root, kind)) == c["json"][root], tag + (root,)
    if not any(c["pending"]):
        _check_depth1(d, c, tag)


def _check_depth1(d, c, tag):
    """The types one level below `tree`, read on their own. A plain object value and a YMap look
    alike in toJSON; map_type_at tells them apart, so the kind comes from there and the text from Yjs."""
    for key, want in c["json"]["tree"].items():
        t = d.map_type_at("tree", key)
        if t == 1:
            assert isinstance(want, dict), tag + (key,)
            assert json.loads(d.type_json("tree", "map", key)) == want, tag + (key,)
        elif t == 0:
            assert isinstance(want, list), tag + (key,)
            assert json.loads(d.type_json("tree", "array", key)) == want, tag + (key,)
        else:
            assert t == -1 and (not isinstance(want, list)), tag + (key,)  # no scalar of the fixture is an array
    for key in ("k0", "k1", "k2", "c", "m", "k"):
        if key not in c["json"]["tree"]:
            assert d.map_type_at("tree", key) == -1, tag + (key,)


@pytest.mark.parametrize("part", range(PARTS))
def test_single_doc_batch_apply(part):
    for c in load()["cases"][part::PARTS]:
        d = crdt_amd.Doc(client_id=ME)
        d.apply_updates(c["updates"])
        _check_doc(d, c, (c["name"],))


@pytest.mark.parametrize("part", range(PARTS))
def test_single_doc_one_at_a_time(part):
    for c in load()["cases"][part::PARTS]:
        d = crdt_amd.Doc(client_id=ME)
        for u in c["updates"]:
            d.apply_update(u)
        _check_doc(d, c, (c["name"],))


# ---------------------------------------------------------------- a batch has no order
@pytest.mark.parametrize("part", range(PARTS))
def test_batch_order_free(part):
    for c in quiet_cases()[part::PARTS]:
        ups = c["updates"]
        want = _single_state(c)
        # the order-free form itself, not merely something that coalesces to it
        assert sha(want[0]) == coalesced(c["state"]) == coalesced(c["state_rev"]), c["name"]
        assert sha(want[1]) == c["sv"], c["name"]
        assert _merge(ups[::-1]) == want, c["name"]
        assert _merge(random.Random(len(ups)).sample(ups, len(ups))) == want, c["name"]
        d = crdt_amd.Doc(client_id=ME)
        d.apply_update(want[0])
        assert d.encode_state_as_update() == want[0], c["name"]
        assert d.pending() == (False, False), c["name"]


# ---------------------------------------------------------------- both merge paths, collisions
def test_merge_paths(path):
    """Three merges each of the forward and the reversed order in one process: all six equal (a
    race between the roots of one nested list shows up as a run that differs) and equal to Yjs."""
    for c in _sampled():
        ups = c["updates"]
        runs = [_merge(order) for order in (ups, ups[::-1]) for _ in range(3)]
        assert all(r == runs[0] for r in runs), c["name"]
        assert_same_update(runs[0][0], c["state"], (c["name"], path))
        assert sha(runs[0][1]) == c["sv"], c["name"]


def test_merge_paths_many_docs(path):
    docs = [c["updates"] for c in _sampled()]
    want = None
    for staged in (docs, [ups[::-1] for ups in docs]):
        for _ in range(2):
            b = crdt_amd.Batch(docs=staged)
            b.merge()
            got = b.result_docs()
            want = want or got
            assert got == want
    for c, (u, sv) in zip(_sampled(), want):
        assert_same_update(u, c["state"], (c["name"], path))
        assert sha(sv) == c["sv"], c["name"]


# ---------------------------------------------------------------- key-hash shards
@pytest.mark.parametrize("nshards", [2, 5])
def test_shards(nshards):
    """A dead ancestor may live in another shard than the list it kills."""
    for c in _sampled():
        assert _merge(c["updates"], nshards) == _single_state(c), c["name"]


# ---------------------------------------------------------------- many documents at once
@pytest.fixture(scope="module")
def fleet():
    """Every case with nothing pending as one document of ONE apply_updates_multi pass."""
    cases = quiet_cases()
    docs = [crdt_amd.Doc(client_id=ME) for _ in cases]
    pairs = [(i, u) for i, c in enumerate(cases) for u in c["updates"]]
    crdt_amd.apply_updates_multi([docs[i] for i, _ in pairs], [u for _, u in pairs])
    return cases, docs


def test_many_docs_ingested_together(fleet):
    cases, docs = fleet
    for c, d in zip(cases, docs):
        assert (d.encode_state_as_update(), d.encode_state_vector()) == _single_state(c), c["name"]


def test_many_docs_one_batch():
    cases = quiet_cases()
    b = crdt_amd.Batch(docs=[c["updates"] for c in cases])
    b.merge()
    for c, got in zip(cases, b.result_docs()):
        assert got == _single_state(c), c["name"]


def test_fleet_json(fleet):
    """docs_json over every document x both roots: Yjs's toJSON, on the device up to the depth
    bound and one by one past it. A dead subtree in a text would differ from Yjs's."""
    cases, docs = fleet
    roots = load()["roots"]
    dmax = crdt_amd.docs_json_stats([], [], [])[1]["depth_max"]
    reqs = [(c, d, root, kind) for c, d in zip(cases, docs) for root, kind in roots.items()]
    texts, st = crdt_amd.docs_json_stats([r[1] for r in reqs], [r[2] for r in reqs], [r[3] for r in reqs])
    deep = sum(c["root_depth"][root] > dmax for c, _, root, _ in reqs)
    assert deep >= 4 and sum(c["root_depth"][root] == dmax for c, _, root, _ in reqs) >= 4  # at the bound and past it
    assert (st["pairs_device"], st["pairs_single"], st["pairs_empty"]) == (len(reqs) - deep, deep, 0), st
    for (c, d, root, kind), t in zip(reqs, texts):
        assert json.loads(t) == c["json"][root], (c["name"], root)
        assert t == d.root_json(root, kind), (c["name"], root)


# ---------------------------------------------------------------- sync replies, lazy merge
def test_sync_replies(fleet):
    cases, docs = fleet
    pairs = [(c, d, r) for c, d in zip(cases, docs) for r in c["diffs"]]
    got = crdt_amd.docs_diff([d for _, d, _ in pairs], [r["sv"] for _, _, r in pairs])
    for (c, d, r), g in zip(pairs, got):
        assert_same_update(g, r["update"], (c["name"], r["sv"].hex()))


def test_merge_updates_equals_yjs():
    for c in load()["cases"]:
        assert sha(crdt_amd.merge_updates(c["updates"])) == c["merged"], c["name"]


# ---------------------------------------------------------------- parked children
def _check_step(d, c, k, st):
    tag = (c["name"], k)
    assert d.pending() == (st["pending"], st["pending_ds"]), tag
    assert_same_update(d.encode_state_as_update(), st["state"], tag)
    assert sha(canonical_sv(d.encode_state_vector())) == st["sv"], tag
    assert_same_update(d.encode_state_as_update(st["delta"]["sv"]), st["delta"]["update"], tag)
    for root, kind in load()["roots"].items():
        assert json.loads(d.root_json(root, kind)) == st["json"][root], tag + (root,)


@pytest.mark.parametrize("part", range(3))
def test_parked_every_step(part):
    """A read after every apply, in shuffled, reversed and one-delta-lost orders: children wait for
    the type item that is their parent exactly as Yjs parks them."""
    for c in load()["parked"][part::3]:
        d = crdt_amd.Doc(client_id=ME)
        for k, (u, st) in enumerate(zip(c["updates"], c["steps"])):
            d.apply_update(u)
            _check_step(d, c, k, st)


def test_parked_deferred_bursts():
    """Reads only every few applies: the deferred queue replays Yjs's sequence."""
    for i, c in enumerate(load()["parked"]):
        d = crdt_amd.Doc(client_id=ME)
        every = 2 + i % 4
        for k, (u, st) in enumerate(zip(c["updates"], c["steps"])):
            d.apply_update(u)
            if k % every == every - 1 or k == len(c["steps"]) - 1:
                _check_step(d, c, k, st)
