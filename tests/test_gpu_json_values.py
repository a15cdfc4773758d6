"""The value text of the fleet toJSON kernels (yc_json.hip k_jsize / k_jplace / k_jwrite over
yc_json.h any_json_text and SegCursor, numbers through yc_num.h) as gfx950 builds it, byte for byte
against truths that share no code with it:

  - Node's recorded JSON.stringify texts (tests/golden/any_json.json, the toJSON records of
    tests/golden/edges.json), the values as list members and as map entries;
  - the exact number reference of tests/jsnum.py (pinned to Node by test_jsnum_reference.py) over
    the double, float32 and decimal-text lists that test_num_text.py runs through the host build;
  - closed-form texts at the 64-level stack bound.

Every comparison is of the UTF-8 bytes of the text: json.loads equality cannot tell 1e21 from 1e+21
or a wrong seventeenth digit, and Doc.root_json is built from the same yc_json.h as the kernels, so
neither is used as the truth here. Every test asserts the routing too (pairs_device, pairs_single,
out_bytes): the device path answered.
"""
import json
import os
import struct
import sys

import pytest

crdt_amd = pytest.importorskip("crdt_amd")
from oracle.yref import Doc as ODoc  # noqa: E402
from tests import jsnum  # noqa: E402
from tests.test_any_json_text import _nest  # noqa: E402
from tests.test_gpu_docs_json import ANY, STRING, anys, doc_of, item, update, vs  # noqa: E402
from tests.test_gpu_json_rewrite import _array_update  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
STRUCT_LENS = (1, 2, 7, 63, 64, 65)
SEPARATORS = "abcdefghijklmnopqrstuvwxyz"


# ---------------------------------------------------------------- helpers
def read(reqs, single=0):
    """docs_json over (doc, root, kind) requests: (texts, stats), the routing asserted."""
    texts, st = crdt_amd.docs_json_stats([d for d, _, _ in reqs], [r for _, r, _ in reqs], [k for _, _, k in reqs])
    assert len(texts) == len(reqs)
    assert st["pairs_device"] == len(reqs) - single, st
    assert st["pairs_single"] == single and st["pairs_empty"] == 0, st
    assert st["out_bytes"] == sum(len(t.encode("utf-8")) for t in texts), st
    return texts, st


def packed_list(root, client, clock, values):
    """`values` — (lib0 any bytes, expected text) pairs — as ContentAny structs of root array `root`,
    their lengths cycling through STRUCT_LENS, a one-character ContentString struct between
    neighbours (nothing merges). Items continue `client` at `clock`.
    -> (items, next clock, [(expected member text, index into values or None)])"""
    items, members = [], []
    k = s = 0
    while k < len(values):
        n = min(STRUCT_LENS[s % len(STRUCT_LENS)], len(values) - k)
        where = dict(root=root) if not items else dict(origin=(client, clock - 1))
        items.append((item(ANY, anys(*[v for v, _ in values[k:k + n]]), **where), n))
        members += [(values[k + j][1], k + j) for j in range(n)]
        clock += n
        k += n
        s += 1
        if k < len(values):
            ch = SEPARATORS[s % len(SEPARATORS)]
            items.append((item(STRING, vs(ch), origin=(client, clock - 1)), 1))
            members.append(('"%s"' % ch, None))
            clock += 1
    return items, clock, members


def assert_members(text, members, describe):
    """text == "[" + members joined + "]"; on a mismatch only the first differing member is shown."""
    want = "[" + ",".join(m for m, _ in members) + "]"
    if text.encode("utf-8") == want.encode("utf-8"):
        return
    assert text[:1] == "[", text[:80]
    pos = 1
    for m, idx in members:
        got = text[pos:pos + len(m)]
        if got != m or text[pos + len(m):pos + len(m) + 1] not in (",", "]"):
            raise AssertionError("%s: expected %r, read back %r" % (describe(idx) if idx is not None else "separator", m, text[pos:pos + len(m) + 8]))
        pos += len(m) + 1
    raise AssertionError("text continues past its last member: %r" % text[pos - 1:pos + 40])


@pytest.fixture(scope="module")
def any_cases():
    with open(os.path.join(HERE, "golden", "any_json.json")) as f:
        cases = json.load(f)["cases"]
    assert len(cases) == 224 and sum(1 for c in cases if c.get("undef")) == 15 and sum(1 for c in cases if "big" in c) == 4
    return cases


def _case_text(c):
    return c["big"] if "big" in c else c["json"]


# ---------------------------------------------------------------- a. Node's fixture as list members
def test_node_fixture_as_list_members(any_cases):
    """Every any_json.json value, in fixture order, as a member of one root array. The fixture is
    laid down 20 times over: 224 is no multiple of the 202 values of one round of struct lengths, so
    every case meets several struct lengths and positions, and the list spans more than 256 segments."""
    values = [(bytes.fromhex(c["any"]), "null" if c.get("undef") else _case_text(c)) for c in any_cases] * 20
    items, _, members = packed_list("a", 51, 0, values)
    assert len(items) > 256
    d = doc_of(update(51, items))
    (text,), _ = read([(d, "a", "array")])
    assert_members(text, members, lambda i: "case " + any_cases[i % len(any_cases)]["name"])


# ---------------------------------------------------------------- b. ... as map entries
def test_node_fixture_as_map_entries(any_cases):
    items = [(item(ANY, anys(bytes.fromhex(c["any"])), root="m", psub="k%04d" % i), 1) for i, c in enumerate(any_cases)]
    d = doc_of(update(52, items))
    (text,), _ = read([(d, "m", "map")])
    entries = [('"k%04d":%s' % (i, _case_text(c)), c["name"]) for i, c in enumerate(any_cases) if not c.get("undef")]
    assert len(entries) == 209
    want = "{" + ",".join(e for e, _ in entries) + "}"
    if text.encode("utf-8") != want.encode("utf-8"):
        pos = 1
        for e, name in entries:
            assert text[pos:pos + len(e)] == e, "case %s: expected %r, read back %r" % (name, e, text[pos:pos + len(e) + 8])
            pos += len(e) + 1
        raise AssertionError("text continues past its last entry: %r" % text[pos - 1:pos + 40])


# ---------------------------------------------------------------- c. the stack bound
def test_any_stack_bound():
    enc64, text64 = _nest(64)
    enc65, text65 = _nest(65)
    at = doc_of(update(53, [(item(ANY, anys(bytes.fromhex(enc64)), root="a"), 1)]))
    past = doc_of(update(54, [(item(ANY, anys(bytes.fromhex(enc64), bytes.fromhex(enc65)), root="a"), 2)]))
    (text,), _ = read([(at, "a", "array")])
    assert text.encode() == ("[" + text64 + "]").encode()
    texts, _ = read([(past, "a", "array"), (at, "a", "array")], single=1)  # 65 levels: the host writer; 64 beside it: the device
    assert texts[0].encode() == ("[" + text64 + "," + text65 + "]").encode()
    assert texts[1].encode() == ("[" + text64 + "]").encode()


def test_deep_nest_in_a_reencoded_struct():
    """What test_node_fixture_as_list_members found: a struct holding a number outside writeAny's form
    (re-encoded when the state is written, yc_work.h any_canon) beside a value nested more than 32
    levels along last members (which the decoder follows without a stack) lost its content — the
    state came out malformed and no toJSON could read it. 2^53 as a float64 (writeAny: float32), a
    40-level nest around a float64 7 (writeAny: the varint 7) and the 64-level nest: the state is that
    of the same struct in writeAny's form, and the text is read on the device."""
    enc40, text40 = _nest(40)
    enc64, text64 = _nest(64)
    assert enc40.endswith("7d00") and text40.count("0") == 1
    nest_raw = bytes.fromhex(enc40[:-4]) + bytes([123]) + struct.pack(">d", 7.0)
    nest_canon = bytes.fromhex(enc40[:-4]) + bytes([125, 7])
    raw = update(56, [(item(ANY, anys(bytes([123]) + struct.pack(">d", 2.0 ** 53), nest_raw, bytes.fromhex(enc64)), root="a"), 3)])
    canon = update(56, [(item(ANY, anys(bytes([124]) + struct.pack(">f", 2.0 ** 53), nest_canon, bytes.fromhex(enc64)), root="a"), 3)])
    oracle = ODoc(0x7FFFFFF0)
    oracle.apply_update(canon)
    d_raw, d_canon = doc_of(raw), doc_of(canon)
    assert d_canon.encode_state_as_update() == oracle.encode_state_as_update()
    assert d_raw.encode_state_as_update() == oracle.encode_state_as_update()
    assert crdt_amd.merge_updates([raw, canon]) == crdt_amd.merge_updates([canon, canon])
    texts, _ = read([(d_raw, "a", "array"), (d_canon, "a", "array")])
    want = "[9007199254740992," + text40.replace("0", "7") + "," + text64 + "]"
    assert texts[0].encode() == want.encode() and texts[1].encode() == want.encode()


# ---------------------------------------------------------------- d. numbers
# values the device build once wrote wrongly, kept by name: (name, double bits) — none so far
FAILED_ONCE = ()


def _storable(bits):
    """A negative integer from -2^32 down to -9.2e18 cannot be stored: lib0's writeVarInt garbles it,
    so the decoder refuses the update (yc_parse.h ANY_UNSUP) and no writer ever meets the value.
    Those of the list are written positive; test_num_text.py keeps them negative."""
    x = jsnum.f64_from(bits)
    return bits & ~(1 << 63) if -9.2e18 <= x <= -4294967296.0 and x == int(x) else bits


def test_numbers_against_reference():
    """The double list (tag 123) and the float32 list (tag 124) in the root arrays of one document,
    2 000 values each at the most, one request per root: the reference texts joined. (The decoder
    stores a float64 that float32 holds exactly as float32 and a small integer as a varint, as Yjs
    would write them back: the value, and so the text, is the same.)"""
    doubles = [(bytes([123]) + struct.pack(">Q", b), jsnum.js_number_text(jsnum.f64_from(b)), "double %016x" % b)
               for b in [_storable(b) for b in jsnum.double_bits()] + [b for _, b in FAILED_ONCE]]
    floats = [(bytes([124]) + struct.pack(">I", b), jsnum.js_number_text(jsnum.f32_from(b)), "float32 %08x" % b)
              for b in [b & 0x7FFFFFFF if _storable(jsnum.f64_bits(jsnum.f32_from(b))) >> 63 == 0 else b for b in jsnum.float32_bits()]]
    assert len(doubles) == 14000 + len(FAILED_ONCE) and len(floats) == 2876
    chunks = [doubles[k:k + 2000] for k in range(0, len(doubles), 2000)] + [floats[k:k + 2000] for k in range(0, len(floats), 2000)]
    items, clock, wants = [], 0, []
    for r, chunk in enumerate(chunks):
        its, clock, members = packed_list("n%d" % r, 55, clock, [(v, t) for v, t, _ in chunk])
        items += its
        wants.append(members)
    d = doc_of(update(55, items))
    texts, _ = read([(d, "n%d" % r, "array") for r in range(len(chunks))])
    for chunk, text, members in zip(chunks, texts, wants):
        assert_members(text, members, lambda i: chunk[i][2])


# ---------------------------------------------------------------- e. the rewrite path
def _short(t):
    return t if len(t) < 80 else t[:40] + "..." + t[-30:]


def test_decimal_texts_rewritten():
    """The decimal texts (all outside Number::toString's form: k_json_canon rewrites each through
    dec_to_f64 and f64_shortest) as ContentJSON values of one large update, beside the same update
    written with the reference texts, which passes through unchanged."""
    raw = jsnum.decimal_texts()
    ref = [jsnum.decimal_expected(t) for t in raw]
    assert len(raw) == 1548 and ref.count("null") >= 3
    # (one step below an integer tie such as 2^53 + 1 is the double itself, already in toString's form: it passes through)
    assert sum(a == b for a, b in zip(raw, ref)) <= 4
    ua, ub = _array_update(4242, [t.encode() for t in raw]), _array_update(4242, [t.encode() for t in ref])
    assert len(ua) > 64 * 1024  # the chunk decoder
    da, db = crdt_amd.Doc(client_id=0x7FFFFFF0), crdt_amd.Doc(client_id=0x7FFFFFF0)
    da.apply_update(ua)
    db.apply_update(ub)
    oracle = ODoc(0x7FFFFFF0)
    oracle.apply_update(ub)
    want_state = oracle.encode_state_as_update()
    sa, sb = da.encode_state_as_update(), db.encode_state_as_update()
    assert sb == want_state
    texts, _ = read([(da, "messages", "array"), (db, "messages", "array")])
    members = [(t, i) for i, t in enumerate(ref)]
    for text in texts:
        assert_members(text, members, lambda i: "text " + _short(raw[i]))
    assert sa == want_state


def test_recorded_json_edges_on_device():
    """The ContentJSON / ContentEmbed / ContentFormat cases of edges.json (duplicate and array-index
    keys, long numbers, deep nests) read through the device path: JSON.stringify of Yjs's recorded
    toJSON, byte for byte."""
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))
    with open(os.path.join(HERE, "golden", "edges.json")) as f:
        cases = [c for c in json.load(f)["cases"] if c["kind"] == "json"]
    assert len(cases) >= 6
    docs = [doc_of(bytes.fromhex(c["update"])) for c in cases]
    reqs = [(d, root, kind) for c, d in zip(cases, docs) for root, kind in c["roots"].items()]
    want = [jsnum.js_stringify(c["json"][root]) for c in cases for root in c["roots"]]
    texts, _ = read(reqs)
    for (c, root), t, w in zip(((c, root) for c in cases for root in c["roots"]), texts, want):
        assert t.encode("utf-8") == w.encode("utf-8"), (c["name"], root, t[:300], w[:300])
    assert any('"insert"' in w for w in want) and any("1.2345678901234568e+29" in w for w in want)
