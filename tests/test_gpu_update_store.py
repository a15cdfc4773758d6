"""The doc-less update store on the GPU: Y.encodeStateVectorFromUpdate for many updates in one device
pass (`ycrdt_updates_state_vectors`, crdt.js:28-77 without the temporary docs) and Y.mergeUpdates per
group for many groups in one device pass (`ycrdt_merge_updates_groups`, the logs of crdt.js:79-98).

References: tests/update_store_ref.sv_from_update (pinned to Yjs 13.5.16 by
tests/test_update_store_ref.py), canonical_update(oracle.ymerge.merge_updates(group)), and the Yjs
bytes recorded in tests/golden/{kat,map,array,nested,merge,update_store}.json. The single calls are
compared as well, but they are not the reference."""
import json
import os
import random
import subprocess
import sys

import pytest

crdt_amd = pytest.importorskip("crdt_amd")
from oracle.ymerge import merge_updates as ref_merge  # noqa: E402
from oracle.yref import Doc as ODoc  # noqa: E402
from tests.histories import any_int, array_history  # noqa: E402
from tests.test_update_store_ref import merge_json_pairs, store_cases  # noqa: E402
from tests.update_store_ref import sv_from_update  # noqa: E402
from tests.v1util import canonical_update  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SETS = ("kat", "map", "array", "nested")


@pytest.fixture(scope="module")
def e135():
    e = crdt_amd.Engine(int(os.environ.get("YCRDT_DEVICE", "0")), compat=135)
    yield e
    e.close()


@pytest.fixture(scope="module")
def sv_inputs(golden):
    """Every update of the four corpora, the new fixture's inputs and Yjs's merges of them (these hold
    the Skips), each with its state vector: (tag, update, reference bytes, Yjs's bytes or None)."""
    rows = []
    for s in SETS:
        for c in golden[s]:
            for i, u in enumerate(c["updates"]):
                b = bytes.fromhex(u)
                rows.append(((s, c["name"], i), b, sv_from_update(b), None))
    for tag, u, sv in merge_json_pairs(golden):
        rows.append((tag, u, sv_from_update(u), bytes.fromhex(sv)))
    for c in store_cases():
        for i, (u, sv) in enumerate(zip(c["updates"], c["svs"])):
            b = bytes.fromhex(u)
            rows.append(((c["name"], i), b, sv_from_update(b), bytes.fromhex(sv)))
        b = bytes.fromhex(c["merged_raw"])
        rows.append(((c["name"], "merged"), b, sv_from_update(b), bytes.fromhex(c["merged_sv"])))
    return rows


def test_state_vectors_one_call(sv_inputs, golden):
    assert len(sv_inputs) > sum(len(c["updates"]) for s in SETS for c in golden[s]) == 2028
    got, st = crdt_amd.state_vectors_from_updates_stats([r[1] for r in sv_inputs])
    assert len(got) == len(sv_inputs)
    for (tag, _, ref, yjs), g in zip(sv_inputs, got):
        assert g == ref, (tag, g.hex(), ref.hex())
        assert yjs is None or g == yjs, (tag, g.hex(), yjs.hex())
    assert st["groups_device"] == len(sv_inputs) and st["groups_single"] == 0 and st["groups_copied"] == 0
    assert st["out_bytes"] == sum(len(g) for g in got)


def test_state_vectors_compat135_same_bytes(sv_inputs, e135):
    rows = [r for r in sv_inputs if r[3] is not None]
    assert crdt_amd.state_vectors_from_updates([r[1] for r in rows], e135) == [r[3] for r in rows]


def test_state_vectors_order_and_repeats(sv_inputs):
    """The result of an update does not depend on its neighbours: reversed order, and the same
    update several times in one call."""
    rows = [r for r in sv_inputs if r[3] is not None][::-1]
    ups = [r[1] for r in rows] + [rows[0][1]] * 3
    got = crdt_amd.state_vectors_from_updates(ups)
    assert got == [r[2] for r in rows] + [rows[0][2]] * 3


def test_single_call_equals_batch(sv_inputs):
    by = {r[0]: r for r in sv_inputs}
    for tag in (("hand_empty_update", 0), ("hand_open_skip_clock0", 0), ("hand_same_client_twice", 0), ("gap_inputs_with_skips", 0),
                ("gap_whole_log", "merged"), ("gc_state", 0), ("ds_only_all", 1), ("diff_vs_A", 0), ("sections_sections_ascending_0", 0)):
        _, u, ref, yjs = by[tag]
        assert crdt_amd.state_vector_from_update(u) == ref == yjs, tag
    assert crdt_amd.state_vector_from_update(b"\x00\x00") == b"\x00"
    assert crdt_amd.state_vectors_from_updates([b"\x00\x00"]) == [b"\x00"]


def test_large_update_and_many_sections():
    """An update past the small-update decode (chunk path) and one with a few hundred sections."""
    big = ODoc(9)
    for k in range(40):
        big.array_insert("messages", k, [any_int(i) for i in range(200)])
    wide = ODoc(1)
    for c in range(2, 300):
        d = ODoc(c)
        d.map_set("users", "k%d" % c, any_int(c))
        wide.apply_update(d.encode_state_as_update())
    ups = [big.encode_state_as_update(), wide.encode_state_as_update(), b"\x00\x00"]
    assert len(ups[0]) > 16384
    assert crdt_amd.state_vectors_from_updates(ups) == [sv_from_update(u) for u in ups]


def test_errors_leave_the_engine_usable(sv_inputs):
    good = [r for r in sv_inputs if r[3] is not None][:5]
    ups = [r[1] for r in good]
    for bad in (b"\x05\xff", b"\x01\x01\x05\x00\x08"):
        with pytest.raises(crdt_amd.YcrdtError) as ei:
            crdt_amd.state_vectors_from_updates(ups[:2] + [bad] + ups[2:])
        assert ei.value.kind == "DECODE", bad
        with pytest.raises(crdt_amd.YcrdtError):
            crdt_amd.state_vector_from_update(bad)
    assert crdt_amd.state_vectors_from_updates(ups) == [r[2] for r in good]
    got, st = crdt_amd.state_vectors_from_updates_stats([])
    assert got == [] and st["groups_device"] == 0 and st["device_ms"] == 0


# ------------------------------------------------------------------ mergeUpdates per group
# References: canonical_update(oracle.ymerge.merge_updates(group)) and the Yjs fixtures. The stats
# say which path a group took: a test that passes through the fallback has not tested the kernel.


def _want(group):
    """What Y.mergeUpdates gives for the group, in the engine's canonical delete-set order."""
    if not group:
        return b"\x00\x00"
    if len(group) == 1:
        return bytes(group[0])  # returned unchanged, as Yjs
    return canonical_update(ref_merge(group))


@pytest.fixture(scope="module")
def corpus(golden):
    """Every kat / map / array / nested case as a group: (tag, updates, Yjs's merged bytes)."""
    rows = []
    for s in SETS:
        for c in golden[s]:
            ups = [bytes.fromhex(u) for u in c["updates"]]
            rows.append(((s, c["name"]), ups, bytes.fromhex(c["merged"] if len(ups) > 1 else c["merged_raw"])))
    assert len(rows) == 202 and sum(len(r[1]) for r in rows) == 2028 and max(len(r[1]) for r in rows) <= 48
    return rows


def _stats_ok(st, n, copied):
    assert st["groups_single"] == 0, st
    assert st["groups_copied"] == copied, st
    assert st["groups_device"] == n - copied, st


def test_groups_golden_corpus_in_case_order(corpus):
    got, st = crdt_amd.merge_update_groups_stats([r[1] for r in corpus])
    _stats_ok(st, len(corpus), sum(len(r[1]) <= 1 for r in corpus))
    for (tag, _, want), g in zip(corpus, got):
        assert g == want, tag
    assert st["out_bytes"] == sum(len(g) for g in got)


def test_groups_golden_corpus_interleaved(corpus):
    """The updates shuffled across groups, each group's own order kept."""
    rng = random.Random(11)
    left = [list(range(len(r[1]))) for r in corpus]
    pick = [g for g, r in enumerate(corpus) for _ in r[1]]
    rng.shuffle(pick)
    flat, gof = [], []
    for g in pick:
        flat.append(corpus[g][1][left[g].pop(0)])
        gof.append(g)
    got, st = crdt_amd.merge_update_groups_stats(flat, group_of=gof, ngroups=len(corpus))
    _stats_ok(st, len(corpus), sum(len(r[1]) <= 1 for r in corpus))
    for (tag, _, want), g in zip(corpus, got):
        assert g == want, tag


def test_groups_reversed_and_pairs_equal_yjs(corpus):
    """merge.json: Yjs's mergeUpdates of the reversed inputs (the reader tie order) and of the first two."""
    with open(os.path.join(HERE, "golden", "merge.json")) as f:
        recs = json.load(f)["cases"]
    by = {r[0]: r[1] for r in corpus}
    groups, want = [], []
    for m in recs:
        ups = by[(m["set"], m["name"])]
        groups.append(ups[::-1])
        want.append(canonical_update(bytes.fromhex(m["rev"])) if len(ups) > 1 else ups[0])
        if "pair" in m:
            groups.append(ups[:2])
            want.append(canonical_update(bytes.fromhex(m["pair"])))
    got, st = crdt_amd.merge_update_groups_stats(groups)
    assert st["groups_single"] == 0 and st["groups_device"] == sum(len(g) > 1 for g in groups)
    assert got == want


def test_groups_store_fixture(corpus):
    """The new fixture's canonical cases (Skips in the inputs, GC, delete-set-only updates, overlapping
    clocks) beside each other; its non-canonical cases are the fallback test's."""
    cases = [c for c in store_cases() if c["kind"] not in ("sections", "hand")]
    groups = [[bytes.fromhex(u) for u in c["updates"]] for c in cases]
    got, st = crdt_amd.merge_update_groups_stats(groups)
    assert st["groups_single"] == 0, st
    for c, grp, g in zip(cases, groups, got):
        assert g == (bytes.fromhex(c["merged"]) if len(grp) > 1 else grp[0]), c["name"]


def _delta(d, op):
    """The update of one transaction on an oracle doc."""
    sv = d.encode_state_vector()
    op(d)
    return d.encode_state_as_update(sv)


def _isolation_groups():
    a = ODoc(5)
    a1 = _delta(a, lambda d: d.array_insert("messages", 0, [any_int(1), any_int(2), any_int(3)]))
    a2 = _delta(a, lambda d: d.array_insert("messages", 3, [any_int(4), any_int(5)]))
    a_full = a.encode_state_as_update()                      # clocks 0..5: overlaps a1 and a2
    a_del = _delta(a, lambda d: d.array_delete("messages", 1, 3))   # delete set only: client 5, clocks 1..4
    assert a_del[0] == 0 and len(a_del) > 2
    b = ODoc(5)                                              # the same client id, another history
    b1 = _delta(b, lambda d: d.map_set("users", "k", any_int(7)))
    b2 = _delta(b, lambda d: d.array_insert("messages", 0, [any_int(9)] * 4))   # abuts b1 (clock 1)
    b_del = _delta(b, lambda d: d.array_delete("messages", 0, 3))   # client 5, clocks 1..4 as well
    c = ODoc(9)
    c1 = _delta(c, lambda d: d.map_set("users", "k", any_int(1)))
    c.apply_update(a_full)
    c2 = _delta(c, lambda d: d.array_delete("messages", 3, 2))      # client 5, clocks 3..5: overlaps a_del
    return [
        [a1, a2, a_full, a_del],     # overlapping clocks, a delete set
        [],                          # an empty group between two non-empty ones
        [b1, b2, b_del, c1],         # client 5 again: abutting clocks, the same delete-set client and clocks
        [a1, a2, a_full, a_del],     # the same update bytes as group 0
        [a_del, c2, b_del],          # only delete sets: overlapping ranges of client 5
        [a_del, c2, a2, c1],         # a hole at client 5's start, client 9 beside it
        [c1],                        # one update: returned unchanged
        [a_full, a1],
    ]


def test_groups_isolation():
    groups = _isolation_groups()
    got, st = crdt_amd.merge_update_groups_stats(groups)
    assert (st["groups_device"], st["groups_single"], st["groups_copied"]) == (6, 0, 2), st
    for i, (grp, g) in enumerate(zip(groups, got)):
        assert g == _want(grp), (i, g.hex(), _want(grp).hex())
        if len(grp) > 1:
            assert g == crdt_amd.merge_updates(grp), i      # (the single call: compared, not the reference)
    assert got[0] == got[3]
    assert crdt_amd.merge_updates([]) == got[1] == b"\x00\x00"
    # one device group alone (a single-document batch)
    got1, st1 = crdt_amd.merge_update_groups_stats([groups[2]])
    assert got1 == [_want(groups[2])] and st1["groups_device"] == 1


def test_groups_random_histories_sharing_client_ids():
    """Six replica histories with the SAME client ids, interleaved: ties, overlaps and delete sets of
    one id in every group."""
    ids = [3, 70000, 2**31 - 5]
    groups = []
    for k in range(6):
        states, wire = array_history(900 + k, n_replicas=3, rounds=3, ops=5, with_map=True, clients=ids)
        groups.append(wire + states if k % 2 else states + wire)
    rng = random.Random(5)
    pick = [g for g, grp in enumerate(groups) for _ in grp]
    rng.shuffle(pick)
    at = [0] * len(groups)
    flat, gof = [], []
    for g in pick:
        flat.append(groups[g][at[g]])
        at[g] += 1
        gof.append(g)
    got, st = crdt_amd.merge_update_groups_stats(flat, group_of=gof, ngroups=len(groups))
    assert st["groups_device"] == 6 and st["groups_single"] == 0, st
    for i, grp in enumerate(groups):
        assert got[i] == _want(grp), i


def _noncanonical_case():
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))  # (edges.json holds 2 000-level JSON values)
    with open(os.path.join(HERE, "golden", "edges.json")) as f:
        c = [c for c in json.load(f)["cases"] if c["kind"] == "sections"][0]
    return [bytes.fromhex(c["update"])] + [bytes.fromhex(u) for u in c["others"]], c


def test_groups_fallback_noncanonical(corpus):
    """One group holds an update whose sections are out of order: that group alone takes the single
    call, the groups around it stay on the device."""
    bad, c = _noncanonical_case()
    around = [r for r in corpus if len(r[1]) > 1][:6]
    groups = [r[1] for r in around[:3]] + [bad] + [r[1] for r in around[3:]] + [[bad[0]]]
    got, st = crdt_amd.merge_update_groups_stats(groups)
    assert (st["groups_device"], st["groups_single"], st["groups_copied"]) == (6, 1, 1), st
    assert got[3].hex() == c["merged_with_others"]
    assert got[3] == _want(bad)
    assert got[7] == bad[0]                                  # one update: unchanged, canonical or not
    for r, g in zip(around, got[:3] + got[4:7]):
        assert g == r[2], r[0]


def test_groups_compat135_all_single(corpus, e135, golden):
    rows = [(c, [bytes.fromhex(u) for u in c["updates"]]) for s in SETS for c in golden[s][:8]]
    got, st = crdt_amd.merge_update_groups_stats([r[1] for r in rows], e135)
    many = sum(len(r[1]) > 1 for r in rows)
    assert (st["groups_device"], st["groups_single"], st["groups_copied"]) == (0, many, len(rows) - many), st
    for (c, _), g in zip(rows, got):
        assert g.hex() == c["merged_raw"], c["name"]


def test_groups_store_switch_off_in_a_child(corpus):
    """YCRDT_STORE=0 (the A/B switch) sends every group through the single call: equal bytes."""
    rows = [r for r in corpus if len(r[1]) > 1][:12]
    code = (
        "import json, sys, crdt_amd\n"
        "groups = [[bytes.fromhex(u) for u in g] for g in json.load(sys.stdin)]\n"
        "got, st = crdt_amd.merge_update_groups_stats(groups)\n"
        "print(json.dumps({'got': [g.hex() for g in got], 'st': st}))\n"
    )
    env = dict(os.environ, YCRDT_STORE="0", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], input=json.dumps([[u.hex() for u in r[1]] for r in rows]), capture_output=True,
                       text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.splitlines()[-1])
    assert out["st"]["groups_single"] == len(rows) and out["st"]["groups_device"] == 0
    assert out["got"] == [r[2].hex() for r in rows]
    assert crdt_amd.merge_update_groups([r[1] for r in rows]) == [r[2] for r in rows]


def test_groups_errors(corpus):
    rows = [r for r in corpus if len(r[1]) > 1][:3]
    groups = [r[1] for r in rows]
    with pytest.raises(crdt_amd.YcrdtError) as ei:
        crdt_amd.merge_update_groups([groups[0], [groups[1][0], b"\x05\xff", groups[1][1]], groups[2]])
    assert ei.value.kind == "DECODE"
    assert crdt_amd.merge_update_groups(groups) == [r[2] for r in rows]   # the engine is usable afterwards
    flat = [u for g in groups for u in g]
    gof = [i for i, g in enumerate(groups) for _ in g]
    with pytest.raises(crdt_amd.YcrdtError) as ei:
        crdt_amd.merge_update_groups_stats(flat, group_of=gof[:-1] + [3], ngroups=3)
    assert ei.value.kind == "ARG"
    got, st = crdt_amd.merge_update_groups_stats([])
    assert got == [] and st["device_ms"] == 0 and st["groups_device"] + st["groups_single"] + st["groups_copied"] == 0
    got, st = crdt_amd.merge_update_groups_stats([[], [], []])
    assert got == [b"\x00\x00"] * 3 and st["groups_copied"] == 3 and st["device_ms"] == 0
