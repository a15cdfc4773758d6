"""Sync replies (ycrdt_docs_diff), CPU side: the fixtures of the real Yjs (tests/golden/sync.json,
gen_sync_fixtures.js) against the oracle, the premise the kernels rest on — everything of a reply
behind the cut struct of a client block, and its delete set, are bytes of the full state — and the
C ABI's argument checks, which need no device."""
import ctypes

import pytest

import crdt_amd
from oracle.yref import Doc as ODoc
from tests.sync_util import blocks, load_cases, parse_sv, reply_from_state
from tests.v1util import canonical_update

CASES = load_cases("sync")


def _pairs():
    for c in CASES:
        for r in c["replies"]:
            if r["update"] is not None:
                yield c, bytes.fromhex(r["sv"]), bytes.fromhex(r["update"])
    for c in load_cases("configs"):
        for r in c["diffs"]:
            yield c, bytes.fromhex(r["sv"]), bytes.fromhex(r["update"])


def test_fixture_covers_the_cut_kinds():
    names = {c["name"] for c in CASES}
    assert {"text_abcd", "text_unicode", "text_pair_inside", "push123", "map_key_reset", "deleted_run", "nested_gc",
            "origin_and_right", "root_first", "big_clients", "wave_steps", "sv_edges"} <= names
    refs = set()
    cut_psub_origin = False
    for c, sv, up in _pairs():
        if c not in CASES:
            continue
        for b in blocks(up)[0]:
            pos, s = b["structs"][0]
            if b["clock"] > 0 and s.kind != 0 and s.origin == (b["client"], b["clock"] - 1):
                refs.add(s.ref)
                cut_psub_origin |= bool(up[pos] & 0x20)
            elif b["clock"] > 0 and s.kind == 0:
                refs.add(0)
    assert {0, 1, 4, 8} <= refs, refs  # GC, Deleted, String, Any cut at an offset
    assert cut_psub_origin  # the parentSub bit on a cut item that has an origin


def test_oracle_reproduces_every_reply():
    for c in CASES:
        o = ODoc(0x7FFFFFF0)
        for u in c["updates"]:
            o.apply_update(bytes.fromhex(u))
        assert canonical_update(o.encode_state_as_update()).hex() == c["state"], c["name"]
        for r in c["replies"]:
            if r["update"] is None:
                assert r["throws"] == "URIError" and c["name"] == "text_pair_inside"
                continue
            got = canonical_update(o.encode_state_as_update(bytes.fromhex(r["sv"])))
            assert got.hex() == r["update"], (c["name"], r["sv"])


def test_reply_tails_and_delete_set_are_state_bytes():
    """Per client block of a reply: the bytes behind its first struct end the state's block of that
    client; a block the peer has nothing of is the state's block whole; the delete set is the
    state's. Reference bytes only."""
    n = 0
    for c, sv, up in _pairs():
        state = bytes.fromhex(c["state"])
        sb, sds = blocks(state)
        by_client = {b["client"]: b for b in sb}
        ub, uds = blocks(up)
        assert up[uds:] == state[sds:], c["name"]
        want = parse_sv(sv)
        assert [b["client"] for b in ub] == [b["client"] for b in sb if want.get(b["client"], 0) < b["end_clock"]]
        for b in ub:
            s = by_client[b["client"]]
            tail = up[b["structs"][1][0]:b["end"]] if b["n"] > 1 else b""
            assert state[s["hdr"]:s["end"]].endswith(tail), (c["name"], sv.hex())
            assert b["end_clock"] == s["end_clock"]
            if b["clock"] <= s["clock"]:
                assert up[b["hdr"]:b["end"]] == state[s["hdr"]:s["end"]]
            n += 1
    assert n > 300


def test_reply_assembled_from_state_bytes():
    """The plan ycrdt_docs_diff follows, on the CPU: a reply assembled from the state's own bytes
    (new header, cut struct re-encoded, the rest copied) is Yjs's reply."""
    for c, sv, up in _pairs():
        assert reply_from_state(bytes.fromhex(c["state"]), sv).hex() == up.hex(), (c["name"], sv.hex())


def test_docs_diff_abi_without_a_device():
    L = crdt_amd.lib()
    assert "ycrdt_docs_diff" in crdt_amd.EXPORTS and hasattr(L, "ycrdt_docs_diff")
    out = crdt_amd._Out()
    offs = (ctypes.c_uint64 * 2)(7, 7)
    docs = (ctypes.c_void_p * 1)()
    svs = (crdt_amd._Buf * 1)()
    fake_engine = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))  # never dereferenced when n == 0
    E_ARG = -6
    assert L.ycrdt_docs_diff(None, docs, svs, 0, ctypes.byref(out), offs, None) == E_ARG
    assert L.ycrdt_docs_diff(fake_engine, None, svs, 0, ctypes.byref(out), offs, None) == E_ARG
    assert L.ycrdt_docs_diff(fake_engine, docs, svs, 0, None, offs, None) == E_ARG
    assert L.ycrdt_docs_diff(fake_engine, docs, svs, 0, ctypes.byref(out), None, None) == E_ARG
    assert L.ycrdt_docs_diff(fake_engine, docs, None, 1, ctypes.byref(out), offs, None) == E_ARG
    assert L.ycrdt_docs_diff(fake_engine, docs, svs, 1, ctypes.byref(out), offs, None) == E_ARG  # a null doc
    assert b"null" in L.ycrdt_last_error()
    st = crdt_amd.SyncStats()
    assert L.ycrdt_docs_diff(fake_engine, docs, svs, 0, ctypes.byref(out), offs, ctypes.byref(st)) == 0
    assert offs[0] == 0 and out.len == 0
    assert st.pairs_marks == st.pairs_walk == st.pairs_single == 0 and st.walk_max > 0
    L.ycrdt_free(ctypes.byref(out))
