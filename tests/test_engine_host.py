"""The pure-host helpers of the engine's host layer (crdt_amd/csrc/yc_engine_host.h): state-vector parsing, the
byte layout of a doc's marks block, and what the calls over many documents share (the bytes of a pass, the
pass windows, 64-byte aligned layouts, the answer blob).
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

CAP = 1 << 31

FLEET = [
    # pass_bytes: the environment's text and the cap; unset, "" and 0 are the cap, nothing exceeds it
    (f"passbytes unset {CAP}", str(CAP)),
    (f"passbytes empty {CAP}", str(CAP)),
    (f"passbytes 0 {CAP}", str(CAP)),
    (f"passbytes 600 {CAP}", "600"),
    (f"passbytes {CAP} {CAP}", str(CAP)),
    (f"passbytes {CAP + 1} {CAP}", str(CAP)),
    (f"passbytes 4294967296 {CAP}", str(CAP)),
    (f"passbytes words {CAP}", str(CAP)),       # (no number: strtoull gives 0)
    # pass_windows: document j joins the window while bytes + len + 64 <= pass_bytes, then
    # bytes += align64(len); the first document of a window is always taken
    ("windows 600 100 100 100", "[0,3)"),       # 128; 128 + 164 = 292, 256; 256 + 164 = 420
    ("windows 600 200 200 200", "[0,2) [2,3)"), # 256; 256 + 264 = 520, 512; 512 + 264 = 776 > 600
    ("windows 600 300 300 300", "[0,1) [1,2) [2,3)"),  # 320; 320 + 364 = 684 > 600, each time
    ("windows 1 5 0 70", "[0,1) [1,2) [2,3)"),  # nothing fits behind another document, an empty one neither
    ("windows 1 7", "[0,1)"),
    ("windows 600 1000", "[0,1)"),              # longer than a pass: its own window
    ("windows 600 1000 10", "[0,1) [1,2)"),
    ("windows 600 10 1000 10", "[0,1) [1,2) [2,3)"),
    ("windows 600 10 10 1000 10 10", "[0,2) [2,3) [3,5)"),
    ("windows 600 64 472", "[0,2)"),            # 64 + 472 + 64 = 600: still in
    ("windows 600 64 473", "[0,1) [1,2)"),      # 601
    ("windows 600 65 408", "[0,2)"),            # the padding counts for the documents in front only: 128 + 408 + 64
    ("windows 600 65 409", "[0,1) [1,2)"),
    ("windows 600", "none"),
    ("windows 1", "none"),
    # Lay: every region on a 64-byte line
    ("lay 1 64 65 0 8", "0 64 128 256 256 size 320"),
    ("lay", "size 0"),
    # pack_blob: offsets, total, the parts back to back; a zero total is a one-byte block
    ("blob", "total 0 offs 0 bytes -"),
    ("blob - - -", "total 0 offs 0 0 0 0 bytes -"),
    ("blob - 0102 - - 03 -", "total 3 offs 0 0 2 2 2 3 3 bytes 010203"),
    ("blob aa", "total 1 offs 0 1 bytes aa"),
    ("blob 7b7d 5b5d 7b7d", "total 6 offs 0 2 4 6 bytes 7b7d5b5d7b7d"),
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
    text = "".join(c + "\n" for c, _ in CASES) + "".join(f"marks {nw} {cap}\n" for nw, cap in MARKS) + "".join(c + "\n" for c, _ in FLEET)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    got = r.stdout.splitlines()
    assert len(got) == len(CASES) + len(MARKS) + len(FLEET)
    for (cmd, want), g in zip(FLEET, got[len(CASES) + len(MARKS):]):
        assert g == want, (cmd, g, want)
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
