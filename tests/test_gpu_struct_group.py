"""k_struct_decode with its workgroup sorted by shape class (yc_shape.h, yc_decode.hip): lane t of a
workgroup decodes struct perm[t], every struct still writes its own columns at its own index. Every
case is compared with the oracle (or the fixture's Yjs bytes) and, in a child process, with the
same case under YCRDT_SD_GROUP=0 (table order, the sort skipped). YCRDT_DECODE_SMALL=0 sends these
small batches through the grid kernels, so k_struct_decode itself runs.

Hand-built updates (one client section each) make struct sequences no editing history gives:
  * one shape, 1 .. 513 structs: a partial last workgroup, lanes past the last struct at the
    barriers, a permutation near the identity;
  * every shape interleaved: struct k takes kind KINDS[(k % P + P * (k // (8 * P))) % len(KINDS)]
    for P = 5 and P = 7 — a cycle of period P through P kinds, the next P kinds after 8 cycles, so
    one workgroup holds every kind;
  * only structs the classifier gives up on (a key that pushes the content out of the 24-byte
    window), and nested `any` values and ContentDoc (the deferred list) in the middle of a
    workgroup;
  * three documents whose structs share workgroups, the lazy merge and diff, a malformed struct
    among valid ones, reduced C1 and C2 batches of the workload generator, and the C3 .. C5
    fixture cases of tests/golden/configs.json (Yjs's own bytes).
"""
import functools
import hashlib
import json
import os
import subprocess
import sys

import pytest

crdt_amd = pytest.importorskip("crdt_amd")
from oracle import ymerge  # noqa: E402
from oracle.yref import Doc as ODoc  # noqa: E402
from tests.histories import array_history  # noqa: E402
from tests.struct_shapes import KINDS, Builder, interleaved, one_shape, only_other, vu, with_deferred  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OBSERVER = 0x7FFFFFF0
COUNTS = (1, 63, 64, 65, 255, 256, 257, 513)


def _sv_of(client, clock):
    return vu(1) + vu(client) + vu(clock)


@functools.lru_cache(maxsize=None)
def _inputs():
    """name -> list of updates of one document."""
    ins = {f"one.{n}": [one_shape(n)] for n in COUNTS}
    ins["p5"] = [interleaved(5, 300, 7)]
    ins["p7"] = [interleaved(7, 300, 9)]
    ins["p5p7"] = [interleaved(5, 300, 7), interleaved(7, 300, 9)]
    ins["other"] = [only_other(300)]
    ins["deferred"] = [with_deferred(300), only_other(40)]
    states, wire = array_history(11, with_map=True)
    ins["history"] = list(states) + list(wire)
    from crdt_amd.workload import gen_map

    ins["c2gen"] = list(gen_map(300, 6, 200, base_snapshot=True)[0])  # C2: mixed values
    ins["c1gen"] = list(gen_map(300, 6, 200, base_snapshot=True, value_mode=1)[0])  # C1: two-member objects
    return ins


def _fixture_cases():
    with open(os.path.join(HERE, "golden", "configs.json")) as f:
        return json.load(f)["cases"]


@functools.lru_cache(maxsize=None)
def _oracle():
    want = {}
    for name, ups in _inputs().items():
        ref = ODoc(OBSERVER)
        for u in ups:
            ref.apply_update(u)
        want[f"{name}.state"], want[f"{name}.sv"] = ref.encode_state_as_update(), ref.encode_state_vector()
    lz = [interleaved(5, 300, 7, lazy=True), interleaved(7, 300, 9, lazy=True)]
    want["lazy.merged"] = ymerge.merge_updates(lz)
    want["lazy.diff0"] = ymerge.diff_update(lz[0], _sv_of(7, 200))
    want["lazy.diff1"] = ymerge.diff_update(lz[1], _sv_of(9, 333))
    for c in _fixture_cases():
        want[f"fx.{c['name']}.state"], want[f"fx.{c['name']}.sv"] = bytes.fromhex(c["state"]), bytes.fromhex(c["sv"])
    return want


def _corrupt_pairs():
    """(name, [valid updates of other shapes, base, refused update]): inputs test_gpu_corrupt.py's
    suite refuses cleanly (an invalid UTF-8 string, an `any` running past the end, ...)."""
    with open(os.path.join(HERE, "golden", "corrupt.json")) as f:
        fx = json.load(f)
    out = []
    for c in fx["cases"]:
        if not c["threw"] or len(out) >= 6:
            continue
        u = bytearray(bytes.fromhex(fx["sources"][c["src"]]))
        bad = bytes(u[: c["cut"]]) if "cut" in c else bytes(u[: c["at"]] + bytes([c["val"]]) + u[c["at"] + 1:])
        out.append((c["name"], [interleaved(5, 300, 7), bytes.fromhex(fx["base"]), bad]))
    return out


def _bad_utf8():
    b = Builder(31, "b")
    for k in range(120):
        b.add(KINDS[k % 5])
    b._list_item(8, vu(1) + bytes([119, 3, 0x61, 0xFF, 0x62]), 1)  # a string that is not UTF-8
    for k in range(120):
        b.add(KINDS[k % 7])
    return b.update()


def _truncated_any():
    b = Builder(33, "t")
    for k in range(70):
        b.add(KINDS[k % 7])
    b._list_item(8, vu(1) + bytes([119, 100, 0x61]), 1)  # a string of 100 bytes, 1 present
    return b.update()[:-1]  # (no delete set: the string runs past the update's end)


def gpu_results():
    """name -> bytes of every case, under whatever YCRDT_SD_GROUP the process runs with."""
    before = os.environ.get("YCRDT_DECODE_SMALL")
    os.environ["YCRDT_DECODE_SMALL"] = "0"  # (read when the batch is staged)
    try:
        return _gpu_results()
    finally:
        if before is None:
            del os.environ["YCRDT_DECODE_SMALL"]
        else:
            os.environ["YCRDT_DECODE_SMALL"] = before


def _gpu_results():
    got = {}
    ins = _inputs()
    for name, ups in ins.items():
        b = crdt_amd.Batch(list(ups))
        b.merge()
        got[f"{name}.state"], got[f"{name}.sv"] = b.result()
    # three small documents whose structs share workgroups
    names = ("one.65", "p7", "history")
    b = crdt_amd.Batch(docs=[list(ins[n]) for n in names])
    b.merge()
    for n, (state, sv) in zip(names, b.result_docs()):
        got[f"multi.{n}.state"], got[f"multi.{n}.sv"] = state, sv
    # the lazy decode (references kept raw, Skip structs inside a section)
    lz = [interleaved(5, 300, 7, lazy=True), interleaved(7, 300, 9, lazy=True)]
    got["lazy.merged"] = crdt_amd.merge_updates(lz)
    got["lazy.diff0"], got["lazy.diff1"] = crdt_amd.diff_updates(lz, [_sv_of(7, 200), _sv_of(9, 333)])
    # refusals: the error kind is the result
    bad = [("badutf8", [interleaved(7, 300, 9), _bad_utf8()]), ("truncated", [interleaved(5, 300, 7), _truncated_any()])]
    for name, ups in bad + _corrupt_pairs():
        try:
            crdt_amd.Batch(ups).merge()
            got[f"refused.{name}"] = b"accepted"
        except crdt_amd.YcrdtError as e:
            got[f"refused.{name}"] = f"refused:{e.kind}".encode()
    for c in _fixture_cases():
        d = crdt_amd.Doc(client_id=OBSERVER)
        d.apply_updates([bytes.fromhex(u) for u in c["updates"]])
        got[f"fx.{c['name']}.state"], got[f"fx.{c['name']}.sv"] = d.encode_state_as_update(), d.encode_state_vector()
    return got


def _expect(name):
    """The oracle entry a GPU result must equal (None: compared across the two settings only)."""
    if name.startswith("multi."):
        return name[len("multi."):]
    return None if name.startswith("refused.") else name


def _digest(b):
    return f"{len(b)}:{hashlib.sha256(b).hexdigest()}"


@functools.lru_cache(maxsize=None)
def _grouped():
    assert os.environ.get("YCRDT_SD_GROUP", "1") != "0"
    return gpu_results()


def test_grouped_matches_oracle():
    got, want = _grouped(), _oracle()
    checked = 0
    for name in sorted(got):
        if _expect(name) is not None:
            assert got[name] == want[_expect(name)], name
            checked += 1
    assert checked >= 2 * (len(_inputs()) + 3) + 3 + 2 * len(_fixture_cases())
    assert {n.split("_")[0] for n in got if n.startswith("fx.")} >= {"fx.c3", "fx.c4", "fx.c5"}


def test_malformed_structs_are_refused():
    got = _grouped()
    refused = {n: v for n, v in got.items() if n.startswith("refused.")}
    assert len(refused) >= 4
    for name, v in refused.items():
        assert v.startswith(b"refused:"), (name, v)
    assert "refused.badutf8" in refused and "refused.truncated" in refused


def test_table_order_gives_the_same_bytes():
    """Every case again in a child process with YCRDT_SD_GROUP=0: the same bytes and the same
    refusals, and the oracle's bytes there too."""
    code = ("import sys, json; sys.path.insert(0, %r)\n"
            "from tests import test_gpu_struct_group as t\n"
            "print(json.dumps({k: t._digest(v) for k, v in t.gpu_results().items()}))\n") % ROOT
    env = dict(os.environ, YCRDT_SD_GROUP="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    child = json.loads(r.stdout.strip().splitlines()[-1])
    grouped = _grouped()
    assert sorted(child) == sorted(grouped)
    for name, dig in child.items():
        assert dig == _digest(grouped[name]), name
        if _expect(name) is not None:
            assert dig == _digest(_oracle()[_expect(name)]), name
