"""The pure-host helpers of the engine's host layer (crdt_amd/csrc/yc_engine_host.h): state-vector parsing and
the byte layout of a doc's marks block.
tests/csrc/engine_host_main.cpp includes the header alone (no HIP), runs one command per line and prints what the
helper gives; the expected lines below are written out by hand. The program is built a second time with
AddressSanitizer and UBSan: every input sits in a heap block of its exact size and the marks block is written
at each of its four offsets, so a read or a layout past the end aborts the run.

State vectors: varuint count, then (client, clock) varuints; 300 = ac 02."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

SORTED = "ok 1:10 5:20 300:7"

CASES = [
    # parse_sv_sorted: one ascending list whatever the order; a client named twice keeps its last clock
    ("sv 03010a0514ac0207", SORTED),            # ascending
    ("sv 03ac02070514010a", SORTED),            # descending (what Yjs writes)
    ("sv 030514ac0207010a", SORTED),            # shuffled
    ("sv 040563010aac02070514", SORTED),        # client 5 twice: 99, then 20
    ("sv 0205630514", "ok 5:20"),               # ... twice in a row
    ("sv 00", "ok"),                            # no entries
    ("sv -", "bad"),                            # no bytes at all (the callers treat a zero length before parsing)
    ("sv 01ac", "bad"),                         # cut inside the client's varuint
    ("sv 02010a05", "bad"),                     # cut before a clock
    ("sv 0180808080800100", "bad"),             # a 6-byte varuint
    ("sv 01808080800800", "ok 2147483648:0"),   # (5 bytes: the largest a 32-bit value needs)
    ("sv 03010a", "bad"),                       # a count larger than the entries present
]

SECTION = 32  # sizeof(yc::Section)
MARKS = [(1, 1), (1, 2), (3, 7)]
MARKS_WANT = {(1, 1): (0, 8, 16, 48, 64), (1, 2): (0, 8, 16, 80, 96), (3, 7): (0, 24, 48, 272, 288)}


def _build(tmp_path, name, extra):
    exe = os.path.join(str(tmp_path), name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-I",
                           os.path.join(ROOT, "crdt_amd", "csrc"), os.path.join(HERE, "csrc", "engine_host_main.cpp"), "-o", exe])
    return exe


def _check(exe):
    text = "".join(c + "\n" for c, _ in CASES) + "".join(f"marks {nw} {cap}\n" for nw, cap in MARKS)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    got = r.stdout.splitlines()
    assert len(got) == len(CASES) + len(MARKS)
    for (cmd, want), g in zip(CASES, got):
        assert g == want, (cmd, g, want)
    for (nw, cap), g in zip(MARKS, got[len(CASES):]):
        f = g.split()
        at = {f[i]: int(f[i + 1]) for i in range(0, len(f), 2)}
        # the order doc_marks allocates for: fbits[nw] | sbits[nw] | secs[cap] | meta (16 bytes), nothing shared
        spans = [(at["fbits"], 8 * nw), (at["sbits"], 8 * nw), (at["secs"], SECTION * cap), (at["meta"], 16)]
        assert spans[0][0] == 0
        for (a, n), (b, _) in zip(spans, spans[1:]):
            assert a + n <= b, (nw, cap, spans)
        assert spans[-1][0] + spans[-1][1] <= at["bytes"] == 16 * nw + SECTION * cap + 16
        assert (at["nw"], at["cap"]) == (nw, cap)
        assert (at["fbits"], at["sbits"], at["secs"], at["meta"], at["bytes"]) == MARKS_WANT[(nw, cap)]


def test_engine_host_helpers(tmp_path):
    _check(_build(tmp_path, "engine_host", []))


def test_engine_host_helpers_sanitized(tmp_path):
    try:
        exe = _build(tmp_path, "engine_host_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    except subprocess.CalledProcessError:
        pytest.fail("the sanitizer build of tests/csrc/engine_host_main.cpp failed")
    _check(exe)
