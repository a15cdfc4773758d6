"""The host view writer of yc_host.cpp (view_root_json, view_type_json, view_map_entries, view_map_get,
view_array_get) over hand-built views: tests/csrc/host_json_main.cpp links yc_host.cpp alone, builds a
HostView from the lines below and prints what every request returns. tests/golden/host_json.json holds
the output of the same program built against yc_host.cpp as it stood before the host and the device
shared one value writer (yc_json.h); the text must come back byte for byte. `python
tests/test_host_json.py <csrc dir>` records the file from the sources in that directory. The program is
built a second time with AddressSanitizer and UBSan: a view's bytes sit in a heap block of their exact
size, so a read past a truncated last segment aborts the run.

Segment flags: 1 deleted, 2 countable, 4 item, 8 set. Content refs: 2 JSON, 3 binary, 4 string, 5 embed,
6 format, 7 type, 8 any, 9 doc."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "host_json.json")

UNDEFINED = "09" + b"undefined".hex()
STR4 = "61c3a9e282acf09f9880"  # a, a 2-byte, a 3-byte and an astral character
DEEP65 = "".join("7501" if i % 2 == 0 else "7601016b" for i in range(65)) + "7d00"

LIST = f"""
S 1 0 2 6 8 10 7d017703616263
S 1 2 2 6 2 12 0131{UNDEFINED}
S 1 4 5 6 4 14 {STR4}
S 1 9 1 7 8 19 -
S 1 10 1 4 6 20 01620474727565
S 1 11 1 6 3 21 03010203
S 1 12 1 6 3 22 00
S 1 13 1 6 5 23 077b2261223a317d
S 1 14 1 6 7 24 01
S 1 15 1 6 7 25 02
S 1 16 1 6 7 26 030170
S 1 17 1 6 9 27 -
S 1 18 1 6 8 28 7f
S 1 19 2 6 8 29 7f7d01
S 1 21 2 6 8 31 7d017f
S 1 23 3 6 8 33 7d017f7d02
S 1 26 3 6 8 36 7d017d027f
S 1 29 1 6 8 39 {DEEP65}
S 1 30 1 6 8 40 7705011f085c22
S 2 0 3 6 4 50 61220a
S 2 3 1 7 4 53 -
S 2 4 2 6 4 54 c3a962
K 0 - a - 0 19
K 1 24 - k 0 0
W 3 0 1 14 8 60 7d07
K 2 25 - - 19 3
I
root a 1
type a - 1
root a 0
root nosuch 1
""" + "".join(f"aget a - {i}\n" for i in range(31))

MAP = f"""
K 0 - m any 0 0
W 1 0 1 14 8 10 7d05
K 1 - m undef 0 0
W 1 1 1 14 8 11 7f
K 2 - m jundef 0 0
W 1 2 1 14 2 12 {UNDEFINED}
K 3 - m json 0 0
W 1 3 1 14 2 13 03227822
K 4 - m str 0 0
W 1 4 5 14 4 14 {STR4}
K 5 - m empty 0 0
W 1 9 0 14 4 19 -
K 6 - m bin0 0 0
W 1 10 1 14 3 20 00
K 7 - m bin3 0 0
W 1 11 1 14 3 21 03010203
K 8 - m embed 0 0
W 1 12 1 14 5 22 077b2261223a317d
K 9 - m fmt 0 0
W 1 13 1 12 6 23 01620474727565
K 10 - m gone 0 0
W 1 14 1 15 8 24 -
K 11 - m unset 0 0
W 0 0 0 0 0 0 -
K 12 - m arr 0 0
W 1 15 1 14 7 40 00
K 13 - m text 0 0
W 1 16 1 14 7 41 02
K 14 - m xml 0 0
W 1 17 1 14 7 42 030170
K 15 - m deep 0 0
W 1 18 1 14 8 44 {DEEP65}
K 16 - m doc 0 0
W 1 19 1 14 9 45 -
K 17 - m map 0 0
W 1 20 1 14 7 43 01
K 18 40 - - 0 2
S 2 0 1 6 7 50 01
S 2 1 1 6 8 51 7a8000000000000000
K 19 50 - k 0 0
W 3 0 1 14 8 60 7d07
K 20 50 - u 0 0
W 3 1 1 14 8 61 7f
K 21 41 - - 2 1
S 2 2 2 6 4 52 6869
K 22 43 - z 0 0
W 3 2 1 14 8 62 78
K 23 43 - f 0 0
W 3 3 1 14 8 63 7c3f8ccccd
I
root m 0
type m - 0
entries m -
root m 1
type m arr 1
type m arr 0
type m map 0
type m map 1
type m any 0
entries m map
entries m arr
aget m arr 0
aget m arr 1
aget m arr 2
aget m map 0
mget m map z
mget m map f
mget m map nokey
mget m arr k
mget m - nokey
""" + "".join(f"mget m - {k}\n" for k in ("any", "undef", "jundef", "json", "str", "empty", "bin0", "bin3", "embed", "fmt",
                                          "gone", "unset", "arr", "text", "xml", "deep", "doc", "map"))

CUT = """
K 1 - a - 0 1
K 0 - m cut 0 0
W 1 0 2 14 4 10 61f09f98
S 1 2 2 6 4 12 61f09f98
I
root m 0
mget m - cut
entries m -
root a 1
aget a - 0
aget a - 1
"""

EMBED_ENTRY = """
K 0 - m e 0 0
W 1 0 1 14 5 10 7f7b
I
root m 0
mget m - e
entries m -
"""

EMBED_MEMBER = """
K 0 - a - 0 2
S 1 0 1 6 8 10 7d01
S 1 1 1 6 5 11 7f7b
I
root a 1
aget a - 0
aget a - 1
"""

CASES = {"list": LIST, "map": MAP, "cut": CUT, "embed_entry": EMBED_ENTRY, "embed_member": EMBED_MEMBER}


def _build(tmp_path, name, extra, csrc=os.path.join(ROOT, "crdt_amd", "csrc")):
    exe = os.path.join(str(tmp_path), name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", *extra, "-I", csrc, "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "csrc", "host_json_main.cpp"), os.path.join(csrc, "yc_host.cpp"), "-o", exe])
    return exe


def _run(exe):
    got = {}
    for name, text in CASES.items():
        r = subprocess.run([exe], input=f"V {name}\n" + text.lstrip("\n"), capture_output=True, text=True,
                           errors="surrogateescape")
        assert r.returncode == 0, (name, r.stdout[-1000:], r.stderr[-3000:])
        got[name] = r.stdout.splitlines()
    return got


def _check(got):
    with open(GOLDEN) as f:
        want = json.load(f)
    assert set(want) == set(CASES)
    for name in CASES:
        for g, w in zip(got[name], want[name]):
            assert g == w, (name, g, w)
        assert len(got[name]) == len(want[name]), name


def test_golden_covers_the_cases():
    with open(GOLDEN) as f:
        want = json.load(f)
    line = {n: {x.split(" => ")[0]: x.split(" => ")[1] for x in want[n][1:]} for n in want}
    for n, text in CASES.items():  # every request has an answer
        assert len(want[n]) == 1 + sum(1 for x in text.splitlines() if x and x[0] not in "SKWI"), n
    assert line["map"]["mget m - undef"] == "2 " and line["map"]["mget m - fmt"] == "2 " and line["map"]["mget m - empty"] == "0 "
    assert line["map"]["mget m - str"] == '1 "\U0001F600"' and line["map"]["mget m - jundef"] == "2 "
    assert line["map"]["mget m - bin3"] == '1 {"0":1,"1":2,"2":3}' and line["map"]["mget m - bin0"] == "1 {}"
    assert line["map"]["type m arr 1"] == '1 [{"k":7},-9223372036854775808]' and line["map"]["mget m map f"] == "1 1.100000023841858"
    assert line["map"]["mget m - text"] == '1 "hi"' and line["map"]["mget m - xml"] == '1 ""' and line["map"]["mget m - doc"] == "1 null"
    assert line["embed_entry"]["root m 0"] == '1 {"e":null}' and line["embed_member"]["root a 1"] == "1 [1,null]"
    assert line["cut"]["root a 1"] == '1 ["a","\udcf0\udc9f\udc98"]' and line["cut"]["mget m - cut"] == '1 "\udcf0\udc9f\udc98"'
    assert line["list"]["aget a - 3"] == "2 " and line["list"]["aget a - 8"] == "0 " and line["list"]["aget a - 30"] == "0 "
    assert line["list"]["aget a - 28"] == r'1 "\u0001\u001f\b\\\""' and line["list"]["aget a - 13"] == '1 "a\\"\\n\u00e9b"'
    assert line["list"]["aget a - 27"] == "1 " + "".join("[" if i % 2 == 0 else '{"k":' for i in range(65)) + "0" + \
        "".join("]" if i % 2 == 0 else "}" for i in reversed(range(65)))
    assert os.path.getsize(GOLDEN) < 100_000


def test_host_view_writer_matches_the_recorded_text(tmp_path):
    _check(_run(_build(tmp_path, "host_json", [])))


def test_host_view_writer_sanitized(tmp_path):
    try:
        exe = _build(tmp_path, "host_json_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    except subprocess.CalledProcessError:
        pytest.fail("the sanitizer build of tests/csrc/host_json_main.cpp failed")
    _check(_run(exe))


if __name__ == "__main__":
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        out = _run(_build(d, "host_json", [], csrc=sys.argv[1]))
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=0, ensure_ascii=True)
        f.write("\n")
