"""tests/golden/text.json (tests/golden/gen/gen_text_fixtures.js): the fixture's own conditions and
the oracle (oracle/yref.c, oracle/ymerge.py) against what Yjs 13.5.16 answered.

A ContentString counts UTF-16 code units. Yjs splits one at origins, delete-set ranges, partly known
duplicates and in mergeUpdates; a split between the two units of a surrogate pair leaves U+FFFD on
both sides (ContentString.splice), while a WRITE at an offset inside a pair (encodeStateAsUpdate(doc,
sv), diffUpdate) throws. A list read gives one element per unit (getContent() is str.split(''))."""
import os

import pytest

from oracle import ymerge
from oracle.yref import Doc as ODoc, OracleError
from tests.text_fixture import PATH, all_cases, by_name, load
from tests.v1util import canonical_sv, canonical_update

ME = 0x7FFFFFF0


def test_fixture_conditions():
    fx = load()
    h = fx["histories"]
    assert os.path.getsize(PATH) <= 500_000
    assert len(h) >= 40
    assert sum(c["pair_split"] for c in h) >= 15 and sum(not c["pair_split"] for c in h) >= 15
    assert sum(c["fmt"] for c in h) >= 10 and sum(c["nested"] for c in h) >= 10
    assert sum(c["kind"] == "safe" for c in h) == sum(c["kind"] == "free" for c in h)
    for c in h + [fx["long"]]:
        assert c["state"] == c["state_rev"], c["name"]  # no history depends on the apply order
        assert not c["pending"] and len(c["replies"]) >= 4, c["name"]
        assert 2 <= c.get("replicas", 2) <= 5
        if not c["pair_split"]:
            assert "�" not in c["json_m"] + c["json_t"], c["name"]
    for c in h:
        assert c["replies"][-1]["sv"] == b"\x00" and len(c["replies"]) == 4, c["name"]
        assert (c["json_t"] == "[]" and c["len_t"] == 0) == c["nested"], c["name"]
    assert [c["name"] for c in all_cases() if c["parks"]] == ["glued_cut_pair_first"]
    assert fx["long"]["len_t"] == 39997 and max(len(u) for u in fx["long"]["updates"]) > 90_000
    # the hand-built answers the issue names
    assert by_name("overlap_inside")["state_raw"].hex() == "0101050004010174066178efbfbd6200"
    assert by_name("overlap_inside")["merged"].hex() == "010205000401017402617884050104efbfbd6200"
    assert by_name("overlap_inside_rev")["json_t"] == r'["a","\ud83d","\ude00","b"]' and by_name("overlap_inside_rev")["len_t"] == 4
    assert by_name("ds_inside")["json_t"] == '["a","�","b"]'
    assert by_name("map_pair_last")["json_m"] == r'{"k":"\ude00"}' and by_name("map_empty")["json_m"] == "{}"
    # Yjs throws only where it writes at an offset inside a pair
    thrown = [(c["name"], r["sv"].hex()) for c in all_cases() for r in c["replies"] if r["update"] is None]
    assert len(thrown) >= 4 and all(n.startswith(("overlap_", "glued", "map_pair")) for n, _ in thrown), thrown


@pytest.mark.parametrize("part", range(4))
def test_oracle_equals_yjs(part):
    """oracle.yref: forward raw (13.5 order) and canonical state, state vector, every recorded reply."""
    for c in all_cases()[part::4]:
        if c["parks"]:  # the oracle does not park structs (tests/golden/pending.json is that ground)
            continue
        o135, o = ODoc(ME, 135), ODoc(ME)
        for u in c["updates"]:
            o135.apply_update(u)
            o.apply_update(u)
        assert o135.encode_state_as_update() == c["state_raw"], c["name"]
        assert o.encode_state_as_update() == c["state"], c["name"]
        assert canonical_sv(o.encode_state_vector()) == c["sv"], c["name"]
        for r in c["replies"]:
            if r["update"] is None:
                with pytest.raises(OracleError):
                    o.encode_state_as_update(r["sv"])
            else:
                assert o.encode_state_as_update(r["sv"]) == r["update"], (c["name"], r["sv"].hex())


@pytest.mark.parametrize("part", range(4))
def test_ymerge_equals_yjs(part):
    """merge_updates writes U+FFFD where it slices a struct inside a pair; diff_update raises where Yjs threw."""
    for c in all_cases()[part::4]:
        ups = c["updates"]
        merged = ymerge.merge_updates(ups)
        assert canonical_update(merged) == c["merged"], c["name"]
        assert canonical_update(ymerge.merge_updates(ups[::-1])) == c["merged_rev"], c["name"]
        for r in c["replies"]:
            if r["diff"] is None:
                with pytest.raises(ValueError):
                    ymerge.diff_update(merged, r["sv"])
            else:
                assert canonical_update(ymerge.diff_update(merged, r["sv"])) == r["diff"], (c["name"], r["sv"].hex())
