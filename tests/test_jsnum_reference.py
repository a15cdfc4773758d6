"""tests/jsnum.py (the number and JSON.stringify reference of the value-writer tests) against Node's
recorded texts, before anything trusts it: every pure-number text of tests/golden/json_forms.json
that JSON.parse accepts, every top-level float of tests/golden/any_json.json, and JSON.stringify of
every any_json.json value. Where the reference and Node's record disagree, Node's record is right
and the reference is wrong."""
import json
import os
import re
import struct

from tests import jsnum

HERE = os.path.dirname(os.path.abspath(__file__))
NUMBER = re.compile(r"-?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)?\Z")

# any_json.json cases whose text Python's str cannot hold as Node wrote it (at most 5 may stand here)
NOT_IN_PYTHON = ()


def _load(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return json.load(f)


def test_number_texts_of_json_forms():
    n = 0
    for w, h, c in _load("json_forms.json")["cases"]:
        text = bytes.fromhex(h).decode("utf-8", "replace")
        if w == 1 or not NUMBER.match(text):
            continue
        want = bytes.fromhex(c).decode() if w == 2 else text
        assert jsnum.js_number_text(float(text)) == want, text
        assert jsnum.js_stringify(json.loads(text)) == want, text
        n += 1
    assert n == 2160


def test_top_level_floats_of_any_json():
    n = 0
    for c in _load("any_json.json")["cases"]:
        raw = bytes.fromhex(c["any"])
        if raw[0] == 123:
            (x,) = struct.unpack(">d", raw[1:9])
        elif raw[0] == 124:
            (x,) = struct.unpack(">f", raw[1:5])
        else:
            continue
        assert jsnum.js_number_text(x) == c["json"], c["name"]
        n += 1
    assert n == 57


def test_stringify_reproduces_any_json():
    assert len(NOT_IN_PYTHON) <= 5
    cases = _load("any_json.json")["cases"]
    assert len(cases) == 224
    n = 0
    for c in cases:
        if c.get("undef") or "big" in c or c["name"] in NOT_IN_PYTHON:
            continue
        assert jsnum.js_stringify(json.loads(c["json"])) == c["json"], c["name"]
        n += 1
    assert n == 224 - 15 - 4 - len(NOT_IN_PYTHON)  # 15 undefined values and 4 BigInts have no JSON text


def test_layout_edges():
    t = jsnum.js_number_text
    assert [t(x) for x in (1e21, 1e-7, 1e-6, 123456789012345680000.0, 5e-324, 0.1 + 0.2, -0.0, float("nan"), float("-inf"))] == [
        "1e+21", "1e-7", "0.000001", "123456789012345680000", "5e-324", "0.30000000000000004", "0", "null", "null"]
    assert jsnum.js_stringify({"a": [1.5, "\n\x1f\ud800\"", None, True, False, {}], "b": []}) == '{"a":[1.5,"\\n\\u001f\\ud800\\"",null,true,false,{}],"b":[]}'


def test_input_lists_are_fixed_and_cover_the_edges():
    bits = jsnum.double_bits()
    assert bits == jsnum.double_bits() and len(bits) == jsnum.N_DOUBLES == len(set(bits))
    mags = {b & ~(1 << 63) for b in bits}
    for e in (-1074, -1023, -1022, 0, 52, 53, 1023):
        b = jsnum.f64_bits(2.0 ** e)
        assert {b, b + 1} <= mags and (b - 1 in mags or b == 1), e
    for _, x in jsnum.NAMED_DOUBLES:
        assert jsnum.f64_bits(x) in mags
    assert 0.2 < sum(b >> 63 for b in bits) / len(bits) < 0.3
    f32 = jsnum.float32_bits()
    assert len(f32) == len(set(f32)) == 828 + jsnum.N_F32_RANDOM  # 277 powers of two with neighbours, three of them shared
    assert {0x00800000, 0x007FFFFF, 0x7F000001, 1} <= {b & 0x7FFFFFFF for b in f32}
    texts = jsnum.decimal_texts()
    assert texts == jsnum.decimal_texts() and len(texts) == 5 * (jsnum.N_DEC_SEEDED + 7) + 13
    assert all(NUMBER.match(s) for s in texts)
    assert max(len(s) for s in texts) > 1600  # a 767-digit tie with its sticky tail
