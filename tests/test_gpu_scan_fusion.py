"""The large-batch passes that number things without a column + scan sandwich, against the oracle
and against the separate passes they replace (YCRDT_SCAN_FUSED=0):

  k_struct_clock_lb  struct clocks as a segmented sum along the struct table (yc_decode.hip)
  k_segments_lb      cut words, their prefix and the segment starts in one tile pass (yc_merge.hip)
  k_popc_scan2       popcount prefixes of the two decode bitmaps in one launch (yc_prims.hip)

The batch is sized just past the one-workgroup limits, so these kernels are the ones that run: one
20 000-unit struct (whole 4 096-unit tiles without a cut), cuts and a 4 100-unit delete run inside
it (longer than a tile), a delta whose single section starts at clock 20 000 and spans more than two
4 096-struct tiles (a tile with no section start: the carry crosses it), a second client, and more
than 1 MiB of bytes (the bitmap prefixes leave k_count_small). The C2 case is the headline's shape:
dense cut words, nearly every unit a segment.
Reference: Y.applyUpdate / encodeStateAsUpdate / encodeStateVector / mergeUpdates (crdt.js:294-305).
"""
import functools
import hashlib
import json
import os
import subprocess
import sys

import pytest

crdt_amd = pytest.importorskip("crdt_amd")
from oracle.yref import Doc as ODoc  # noqa: E402
from tests.histories import any_int  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBSERVER = 0x7FFFFFF0


def _val(tag, i):
    # 800-byte strings: an encode keeps only the ~1 200 live map values (an overwritten one is a
    # ContentDeleted of a few bytes), and those have to carry the batch past 1 MiB
    b = (f"{tag}-{i:06d}-" + "x" * 800)[:800].encode()
    return bytes([119, 0x80 | (len(b) & 0x7F), len(b) >> 7]) + b  # lib0 any: string, varuint length


@functools.lru_cache(maxsize=None)
def _updates(tag):
    """(u1, u2, u3, sv1): A's 20 000-value insert; A's deletes + 9 000 map sets as a delta; B's
    6 000 map sets + a 5-value insert at 7 000 as a delta."""
    a = ODoc(1001)
    a.array_insert("messages", 0, [any_int(i % 1000) for i in range(20000)])
    u1, sv1 = a.encode_state_as_update(), a.encode_state_vector()
    a.array_delete("messages", 5000, 3)
    a.array_delete("messages", 9000, 4100)
    for i in range(9000):
        a.map_set("users", f"user{(i * 7919) % 700}", _val(tag + "a", i))
    u2 = a.encode_state_as_update(sv1)
    b = ODoc(2002)
    b.apply_update(u1)
    for i in range(6000):
        b.map_set("users", f"user{(i * 104729) % 500}", _val(tag + "b", i))
    b.array_insert("messages", 7000, [any_int(i) for i in range(5)])
    u3 = b.encode_state_as_update(sv1)
    assert len(u1) + len(u2) + len(u3) > (1 << 20) + 4096  # past COUNT_SMALL words of bitmap
    return u1, u2, u3, sv1


@functools.lru_cache(maxsize=None)
def _c2():
    from crdt_amd.workload import gen_map

    ups, _ = gen_map(2000, 24, 1500, base_snapshot=True)
    return tuple(ups)


def _oracle_of(updates):
    ref = ODoc(OBSERVER)
    for u in updates:
        ref.apply_update(u)
    return ref


@functools.lru_cache(maxsize=None)
def _oracle():
    """name -> the bytes every GPU result of that name must equal."""
    want = {}
    for tag in ("d0", "d1", "d2"):
        u1, u2, u3, sv1 = _updates(tag)
        ref = _oracle_of((u1, u2, u3))
        want[f"{tag}.state"], want[f"{tag}.sv"] = ref.encode_state_as_update(), ref.encode_state_vector()
        if tag == "d0":
            want["d0.delta"] = ref.encode_state_as_update(sv1)
    ref = _oracle_of(_c2())
    want["c2.state"], want["c2.sv"] = ref.encode_state_as_update(), ref.encode_state_vector()
    return want


def gpu_results():
    """name -> bytes of every case, under whatever YCRDT_SCAN_FUSED the process runs with."""
    got = {}
    u1, u2, u3, sv1 = _updates("d0")
    for name, ups in (("fwd", [u1, u2, u3]), ("rev", [u3, u2, u1])):
        b = crdt_amd.Batch(ups)
        st = b.merge()
        got[f"{name}.state"], got[f"{name}.sv"] = b.result()
        # past the one-workgroup paths (k_decode_tail_small, k_segments_small)
        assert st.structs > 4096 and st.units > 16384, st.as_dict()
    d = crdt_amd.Doc(client_id=OBSERVER)
    d.apply_updates([u1, u2, u3])
    got["doc.state"], got["doc.sv"] = d.encode_state_as_update(), d.encode_state_vector()
    got["doc.delta"] = d.encode_state_as_update(sv1)  # a delta encode against u1's state vector
    # the headline's multi-document path: three documents in one pass
    docs = [list(_updates(tag)[:3]) for tag in ("d0", "d1", "d2")]
    b = crdt_amd.Batch(docs=docs)
    b.merge()
    for tag, (state, sv) in zip(("d0", "d1", "d2"), b.result_docs()):
        got[f"multi.{tag}.state"], got[f"multi.{tag}.sv"] = state, sv
    # lazy mode (mergeUpdates), then the doc-state path: a fresh Doc applies the merged update, and
    # another applies that Doc's state
    merged = crdt_amd.merge_updates([u1, u2, u3])
    got["lazy.merged"] = merged
    d1 = crdt_amd.Doc(client_id=OBSERVER)
    d1.apply_update(merged)
    got["lazy.state"], got["lazy.sv"] = d1.encode_state_as_update(), d1.encode_state_vector()
    d2 = crdt_amd.Doc(client_id=OBSERVER)
    d2.apply_update(got["lazy.state"])
    got["state.state"], got["state.sv"] = d2.encode_state_as_update(), d2.encode_state_vector()
    b = crdt_amd.Batch(list(_c2()))
    b.merge()
    got["c2.state"], got["c2.sv"] = b.result()
    return got


# GPU result -> the oracle entry it must equal (lazy.merged: no oracle entry, compared across settings)
EXPECT = {
    "fwd.state": "d0.state", "fwd.sv": "d0.sv", "rev.state": "d0.state", "rev.sv": "d0.sv",
    "doc.state": "d0.state", "doc.sv": "d0.sv", "doc.delta": "d0.delta",
    "multi.d0.state": "d0.state", "multi.d0.sv": "d0.sv", "multi.d1.state": "d1.state", "multi.d1.sv": "d1.sv",
    "multi.d2.state": "d2.state", "multi.d2.sv": "d2.sv",
    "lazy.state": "d0.state", "lazy.sv": "d0.sv", "state.state": "d0.state", "state.sv": "d0.sv",
    "c2.state": "c2.state", "c2.sv": "c2.sv",
}


def _digest(b):
    return f"{len(b)}:{hashlib.sha256(b).hexdigest()}"


@functools.lru_cache(maxsize=None)
def _fused():
    assert os.environ.get("YCRDT_SCAN_FUSED", "1") != "0"
    return gpu_results()


@pytest.mark.parametrize("name", sorted(EXPECT))
def test_fused_matches_oracle(name):
    assert _fused()[name] == _oracle()[EXPECT[name]], name


def test_separate_passes_give_the_same_bytes():
    """Every case again in a child process with YCRDT_SCAN_FUSED=0: the oracle's bytes, and the
    lazy merge's bytes identical under both settings."""
    code = ("import sys, json; sys.path.insert(0, %r)\n"
            "from tests import test_gpu_scan_fusion as t\n"
            "print(json.dumps({k: t._digest(v) for k, v in t.gpu_results().items()}))\n") % ROOT
    env = dict(os.environ, YCRDT_SCAN_FUSED="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    child = json.loads(r.stdout.strip().splitlines()[-1])
    fused = _fused()
    assert sorted(child) == sorted(fused)
    for name, dig in child.items():
        assert dig == _digest(fused[name]), name
        if name in EXPECT:
            assert dig == _digest(_oracle()[EXPECT[name]]), name


def _vu(v):
    out = bytearray()
    while v > 0x7F:
        out.append(0x80 | (v & 0x7F))
        v >>= 7
    out.append(v)
    return bytes(out)


@pytest.mark.parametrize("clock,length", [(0xFFFFF000, 1), (0, 0x7FFFFFFF)])
def test_clock_past_u32_is_refused_the_same_way(monkeypatch, clock, length):
    """One section of 6 000 GC structs whose clocks run past 2^32 (Yjs clocks are u32): at the last
    struct of the first 4 096-struct tile, or within the first few structs so that the tile carry
    saturates. Both the single pass and the separate passes refuse the update with the same error."""
    n = 6000
    upd = _vu(1) + _vu(n) + _vu(77) + _vu(clock) + (bytes([0]) + _vu(length)) * n + bytes([0])
    kinds = []
    for fused in ("1", "0"):
        monkeypatch.setenv("YCRDT_SCAN_FUSED", fused)
        with pytest.raises(crdt_amd.YcrdtError) as ei:
            crdt_amd.Batch([upd]).merge()
        kinds.append(ei.value.kind)
    assert kinds[0] == kinds[1], kinds
