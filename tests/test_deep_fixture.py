"""tests/golden/deep.json on the CPU: what the recorded histories contain (a census with floors,
so a regenerated file cannot quietly lose the deep cases), the oracle against Yjs 13.5.16 on them,
and the comparison rule the GPU tests use (tests/deep_fixture.py, tests/v1util.py coalesce_gc).

The fixture records Yjs applying every case's updates forward and reversed. Where nothing is
pending the two states differ only in how adjacent GC structs of a client are cut; coalesce_gc
removes exactly that difference and is tested here on hand-written bytes first.
"""
import json

from oracle.ymerge import merge_updates
from tests.deep_fixture import coalesced, exact, is_random, load, quiet_cases, sha
from tests.v1util import canonical_sv, canonical_update, coalesce_gc, delete_set_of


# ---------------------------------------------------------------- coalesce_gc on hand-written bytes
def vu(n):
    out = bytearray()
    while n > 127:
        out.append(128 | (n & 127))
        n >>= 7
    out.append(n)
    return bytes(out)


def gc(n):
    return bytes([0]) + vu(n)


def skip(n):
    return bytes([10]) + vu(n)


def item(v, origin=None):
    """One ContentAny item of root "r" holding the small integer v (or with an origin id)."""
    if origin:
        return bytes([0x88]) + vu(origin[0]) + vu(origin[1]) + vu(1) + bytes([125, v])
    return bytes([8, 1, 1]) + b"r" + vu(1) + bytes([125, v])


def section(client, clock, *structs):
    return vu(len(structs)) + vu(client) + vu(clock) + b"".join(structs)


def update(sections, ds=b"\x00"):
    return vu(len(sections)) + b"".join(sections) + ds


DS = vu(1) + vu(7) + vu(2) + vu(0) + vu(2) + vu(300) + vu(1)  # client 7: (0, 2) and (300, 1), unmerged


def test_coalesce_no_gc():
    u = update([section(7, 0, item(1), item(2, (7, 0)))], DS)
    assert coalesce_gc(u) == u
    assert coalesce_gc(b"\x00\x00") == b"\x00\x00"


def test_coalesce_one_run():
    u = update([section(7, 3, item(1), gc(200), item(2, (7, 3)))], DS)
    assert coalesce_gc(u) == u


def test_coalesce_run_split_in_three():
    u = update([section(7, 0, item(1), gc(1), gc(1), gc(3), item(2, (7, 0)), gc(127), gc(1))], DS)
    want = update([section(7, 0, item(1), gc(5), item(2, (7, 0)), gc(128))], DS)
    assert coalesce_gc(u) == want
    assert coalesce_gc(want) == want
    assert delete_set_of(coalesce_gc(u)) == delete_set_of(u) == {7: [(0, 2), (300, 1)]}


def test_coalesce_gc_beside_skip():
    u = update([section(7, 0, gc(2), gc(1), skip(4), gc(1), gc(1), skip(1), skip(1))])
    assert coalesce_gc(u) == update([section(7, 0, gc(3), skip(4), gc(2), skip(1), skip(1))])


def test_coalesce_two_clients():
    """A run ends at the client boundary even where the clocks would continue."""
    u = update([section(9, 0, gc(1), gc(2)), section(7, 3, gc(1), gc(1), item(5, (9, 0)))], DS)
    assert coalesce_gc(u) == update([section(9, 0, gc(3)), section(7, 3, gc(2), item(5, (9, 0)))], DS)


# ---------------------------------------------------------------- the committed file
def _order_dependent():
    return [c for c in quiet_cases() if c["state"] != c["state_rev"]]


def test_census():
    fx = load()
    cases = fx["cases"]
    rnd = [c for c in cases if is_random(c)]
    per_history = fx["histories"]
    assert len(per_history) >= 55 and len(rnd) == 3 * len(per_history)
    assert sum(h["subtree_deletes"] for h in per_history) >= 100
    assert sum(h["orphan_inserts"] for h in per_history) >= 100
    assert sum(h["types_in_arrays"] for h in per_history) >= 300
    assert sum(c["live_depth"] >= 4 for c in rnd) >= 8
    assert sum(c["live_depth"] >= 5 for c in cases) >= 3
    assert sum(c["gc_in_input"] > 0 for c in cases) >= 50
    assert len(_order_dependent()) >= 10
    assert len(fx["parked"]) == 36
    for c in fx["parked"]:
        assert c["parked_steps"] == sum(s["parked"] for s in c["steps"]) and len(c["steps"]) == len(c["updates"])
    assert sum(c["parked_steps"] for c in fx["parked"]) >= 20
    names = {c["name"] for c in cases}
    want = {f"chain_d{n}{cut}" for n in range(1, 7) for cut in ("", "_cut")}
    want |= {"range_kills_tree", "many_roots_nested_live", "many_roots_nested_dead", "rival_types", "gc_parent"}
    assert want <= names


def test_hand_built_shapes():
    """The hand-built histories are what their names say."""
    by = {c["name"]: c for c in load()["cases"]}
    for n in range(1, 7):
        assert by[f"chain_d{n}"]["live_depth"] == n
        assert by[f"chain_d{n}_cut"]["live_depth"] == 0
        assert by[f"chain_d{n}_cut"]["json"]["tree"] == {"c": "gone", "v": 0, "w": "late0"}
    assert by["range_kills_tree"]["json"] == {"tree": {}, "list": []}
    live, dead = by["many_roots_nested_live"], by["many_roots_nested_dead"]
    assert len(live["updates"]) == 301 and sorted(live["json"]["tree"]["m"]["arr"]) == list(range(300))
    assert len(dead["updates"]) == 302 and dead["json"]["tree"] == {"m": 0}
    assert by["rival_types"]["json"]["tree"] == {"k": {}}
    assert by["gc_parent"]["json"]["tree"] == {} and by["gc_parent"]["gc_in_input"] > 0


def test_oracle_equals_yjs_forward():
    """Sequential apply in the recorded order: Yjs's forward bytes exactly, no coalescing; so do the
    replies to the recorded state vectors. Where Yjs's bytes are not in the order-free form, the
    coalescer here and the generator's give the same bytes."""
    from oracle.yref import Doc as ODoc

    fx = load()
    for c in quiet_cases():
        o = ODoc(0x7FFFFFF0)
        for u in c["updates"]:
            o.apply_update(u)
        for got, want in [(o.encode_state_as_update(), c["state"])] + [(o.encode_state_as_update(r["sv"]), r["update"]) for r in c["diffs"]]:
            assert sha(got) == (want if exact(want) else want[0]), c["name"]
            assert sha(coalesce_gc(got)) == coalesced(want), c["name"]
            assert exact(want) == (coalesce_gc(got) == got), c["name"]
        assert sha(canonical_sv(o.encode_state_vector())) == c["sv"], c["name"]
        for root, kind in fx["roots"].items():
            assert json.loads(o.root_json(root, kind)) == c["json"][root], (c["name"], root)


def test_coalesced_states_are_order_free_and_mostly_exact():
    quiet = quiet_cases()
    for c in quiet:
        assert coalesced(c["state"]) == coalesced(c["state_rev"]), c["name"]
    inexact = [c["name"] for c in quiet if not exact(c["state"])]
    print(f"deep.json: {len(quiet)} cases with nothing pending, {len(quiet) - len(inexact)} compared exactly, "
          f"{len(inexact)} only coalesced, {len(_order_dependent())} order dependent in Yjs")
    assert 4 * len(inexact) <= len(quiet), inexact
    for c in _order_dependent():  # what differs is the cut of GC runs, nothing else
        assert not (exact(c["state"]) and exact(c["state_rev"])), c["name"]


def test_lazy_merge_equals_yjs():
    for c in load()["cases"]:
        assert sha(canonical_update(merge_updates(c["updates"]))) == c["merged"], c["name"]
