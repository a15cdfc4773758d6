"""tests/update_store_ref.sv_from_update (the CPU restatement of Y.encodeStateVectorFromUpdate) against
Yjs 13.5.16's own bytes — the reference the GPU tests of the update store compare with:

* tests/golden/merge.json: its generator called Yjs's encodeStateVectorFromUpdate on the first and the
  last update of every case to make the state vectors it diffs against (`diffs[].sv` entries 1 and 2
  of `src == "merged"`): 141 (update, state vector) pairs;
* tests/golden/update_store.json (gen_update_store_fixtures.js): inputs the old corpus lacks — diffs
  that start past clock 0, merges with Skips, GC structs, delete-set-only updates, overlapping
  clocks, hand-written layouts Yjs reads but never writes, the non-canonical updates of edges.json.
  The same file pins oracle.ymerge.merge_updates on those inputs."""
import json
import os

import pytest

from oracle.ymerge import GC, SKIP, Dec, lazy_structs, merge_updates
from tests.update_store_ref import sv_from_update
from tests.v1util import canonical_update

HERE = os.path.dirname(os.path.abspath(__file__))


def merge_json_pairs(golden):
    """(tag, update, Yjs's state vector of it) from merge.json and the corpora it was made from."""
    with open(os.path.join(HERE, "golden", "merge.json")) as f:
        recs = json.load(f)["cases"]
    by_name = {(s, c["name"]): c for s, cases in golden.items() for c in cases}
    out = []
    for r in recs:
        ups = by_name[(r["set"], r["name"])]["updates"]
        svs = [d["sv"] for d in r["diffs"] if d["src"] == "merged"]
        assert svs[0] == "00" and len(svs) == (3 if len(ups) >= 2 else 2), r["name"]
        out.append(((r["set"], r["name"], "first"), bytes.fromhex(ups[0]), svs[1]))
        if len(ups) >= 2:
            out.append(((r["set"], r["name"], "last"), bytes.fromhex(ups[-1]), svs[2]))
    return out


def store_cases():
    with open(os.path.join(HERE, "golden", "update_store.json")) as f:
        return json.load(f)["cases"]


def test_merge_json_pairs(golden):
    pairs = merge_json_pairs(golden)
    assert len(pairs) == 141
    for tag, u, sv in pairs:
        assert sv_from_update(u).hex() == sv, tag


def test_fixture_state_vectors():
    for c in store_cases():
        for i, (u, sv) in enumerate(zip(c["updates"], c["svs"])):
            assert sv_from_update(bytes.fromhex(u)).hex() == sv, (c["name"], i)
        assert sv_from_update(bytes.fromhex(c["merged_raw"])).hex() == c["merged_sv"], c["name"]
        assert sv_from_update(bytes.fromhex(c["merged"])).hex() == c["merged_sv"], c["name"]  # (the delete set is not read)


def test_fixture_merges():
    for c in store_cases():
        ups = [bytes.fromhex(u) for u in c["updates"]]
        assert canonical_update(merge_updates(ups)).hex() == c["merged"], c["name"]


def test_fixture_covers_what_it_claims():
    """The shapes the fixture exists for are in it (a regenerated file that lost one fails here)."""
    cases = store_cases()
    kinds = {c["kind"] for c in cases}
    assert kinds == {"diff", "gaps", "gc", "ds_only", "overlap", "hand", "sections"}
    structs = {c["name"]: [lazy_structs(Dec(bytes.fromhex(u))) for u in c["updates"] + [c["merged_raw"]]] for c in cases}
    first_clock_past_0 = mid_skip = gc = ds_only = 0
    for c in cases:
        for u, st in zip(c["updates"] + [c["merged_raw"]], structs[c["name"]]):
            first_clock_past_0 += bool(st) and st[0].clock != 0
            mid_skip += any(s.kind == SKIP and 0 < i < len(st) - 1 for i, s in enumerate(st))
            gc += any(s.kind == GC for s in st)
            ds_only += not st and len(u) > 4
    assert first_clock_past_0 >= 4 and mid_skip >= 3 and gc >= 2 and ds_only >= 2
    by = {c["name"]: c for c in cases}
    assert by["hand_empty_update"]["svs"] == ["00"]
    assert by["hand_open_skip_clock0"]["svs"] == ["010503"]         # the first struct's end, though it is a Skip
    assert by["hand_same_client_twice"]["svs"] == ["010508"]        # two sections of one client: one run
    assert by["hand_skip_first_in_second_client"]["svs"] == ["010901"]
    assert os.path.getsize(os.path.join(HERE, "golden", "update_store.json")) < 64 * 1024


@pytest.mark.parametrize("bad", ["", "01", "0101050008", "01010500"])
def test_malformed_raises(bad):
    with pytest.raises(ValueError):
        sv_from_update(bytes.fromhex(bad))
