"""The host build of the number writers against the exact reference of tests/jsnum.py: yc_json.h
json_put_number (a double -> Number::toString's text, yc_num.h f64_shortest and num_text) over the
double and float32 lists, yc_num.h json_number_canon (a number text -> JSON.stringify(JSON.parse(text)),
dec_to_f64 first) over the decimal texts. tests/csrc/num_text_main.cpp is built with g++ twice,
plain and with AddressSanitizer and UBSan, as test_any_json_text.py builds its program.

This is the CPU half of test_gpu_json_values.py, which runs the same lists through the device
build: when that one fails, this one tells a wrong algorithm from a wrong device build."""
import os
import subprocess

import pytest

from tests import jsnum

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", *extra, "-I", os.path.join(ROOT, "crdt_amd", "csrc"),
                           os.path.join(HERE, "csrc", "num_text_main.cpp"), "-o", str(exe)])
    return exe


@pytest.fixture(scope="module")
def inputs():
    """(input line, expected text, what to show on a mismatch) for every value of the shared lists"""
    rows = []
    for b in jsnum.double_bits():
        rows.append(("D %016x" % b, jsnum.js_number_text(jsnum.f64_from(b)), "double %016x" % b))
    for b in jsnum.float32_bits():
        rows.append(("F %08x" % b, jsnum.js_number_text(jsnum.f32_from(b)), "float32 %08x" % b))
    for t in jsnum.decimal_texts():
        rows.append(("N " + t, jsnum.decimal_expected(t), "text " + (t if len(t) < 80 else t[:40] + "..." + t[-30:])))
    assert len(rows) == 14000 + 2876 + 1548
    return rows


def _check(exe, rows):
    r = subprocess.run([str(exe)], input="".join(line + "\n" for line, _, _ in rows), capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    out = r.stdout.splitlines()
    assert len(out) == len(rows)
    for got, (_, want, what) in zip(out, rows):
        assert got == want, what


def test_number_writers_match_reference(tmp_path, inputs):
    _check(_build(tmp_path, "num_text", []), inputs)


def test_number_writers_sanitized(tmp_path, inputs):
    try:
        exe = _build(tmp_path, "num_text_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    except subprocess.CalledProcessError:
        pytest.fail("the sanitizer build of tests/csrc/num_text_main.cpp failed")
    _check(exe, inputs)
