"""yc_str.h and SegCursor on the host: a ContentString piece cut by UTF-16 units, as Yjs holds it.

Yjs splits a string between the two units of a surrogate pair and ContentString.splice leaves
U+FFFD on both sides; the engine keeps such a piece as 3 of the character's 4 bytes and every
writer and reader takes them for EF BF BD (DESIGN.md §3 "Text content"). Every string of 1 to 4
characters over {a, é, €, 😀} (1- to 4-byte UTF-8; 340 strings) is cut at every 0 <= e0 < e1 <= units
and compared with Python's own arithmetic on the UTF-16 units: the written bytes, the refusal of an
offset Yjs writes at (lib0 throws inside a pair), the text inside a YText's JSON, and the SegCursor
elements as a list and as a map entry's value. tests/csrc/str_piece_main.cpp is built plain and with
AddressSanitizer and UBSan: the text sits in a heap block of its exact size and the piece is written
into a block of exactly its sliced size."""
import itertools
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

ALPHABET = ["a", "é", "€", "\U0001F600"]
STRINGS = ["".join(t) for n in range(1, 5) for t in itertools.product(ALPHABET, repeat=n)]


def units(s):
    b = s.encode("utf-16-le")
    return [int.from_bytes(b[i:i + 2], "little") for i in range(0, len(b), 2)]


def piece(s, e0, e1):
    """Units [e0, e1) of s as characters: a lone half at either edge is U+FFFD."""
    u = units(s)[e0:e1]
    text = b"".join(x.to_bytes(2, "little") for x in u).decode("utf-16-le", errors="surrogatepass")
    chars = list(text)
    for i in (0, -1):
        if 0xD800 <= ord(chars[i]) <= 0xDFFF:
            chars[i] = "�"
    assert not any(0xD800 <= ord(c) <= 0xDFFF for c in chars)  # only an edge can be cut
    return chars


def inside_pair(s, e):
    u = units(s)
    return 0 < e < len(u) and 0xDC00 <= u[e] <= 0xDFFF


CUTS = [(s, e0, e1) for s in STRINGS for e0 in range(len(units(s))) for e1 in range(e0 + 1, len(units(s)) + 1)]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("str_piece")
    out = {}
    for name, extra in (("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = d / name
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", *extra, "-I", os.path.join(ROOT, "crdt_amd", "csrc"),
                               os.path.join(HERE, "csrc", "str_piece_main.cpp"), "-o", str(exe)])
        out[name] = exe
    return out


def _run(exe, mode):
    lines = [f"{mode} {s.encode().hex()} {e0} {e1}" for s, e0, e1 in CUTS]
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def test_inputs():
    assert len(STRINGS) == 340
    assert any(inside_pair(s, e0) and inside_pair(s, e1) for s, e0, e1 in CUTS)  # both edges cut
    assert any(e1 - e0 == 1 and (inside_pair(s, e0) or inside_pair(s, e1)) for s, e0, e1 in CUTS)  # a piece that is one half


@pytest.mark.parametrize("build", ["plain", "san"])
def test_split_bytes(programs, build):
    for (s, e0, e1), line in zip(CUTS, _run(programs[build], "S")):
        assert line == "".join(piece(s, e0, e1)).encode().hex(), (s, e0, e1, line)


@pytest.mark.parametrize("build", ["plain", "san"])
def test_write_offset(programs, build):
    refused = 0
    for (s, e0, e1), line in zip(CUTS, _run(programs[build], "W")):
        if inside_pair(s, e0):
            assert line == "refused", (s, e0, e1, line)
            refused += 1
        else:  # (the end is a struct's or a segment's: a split)
            assert line == "".join(piece(s, e0, e1)).encode().hex(), (s, e0, e1, line)
    assert refused


@pytest.mark.parametrize("build", ["plain", "san"])
def test_ytext_member(programs, build):
    for (s, e0, e1), line in zip(CUTS, _run(programs[build], "T")):
        assert line == "".join(piece(s, e0, e1)).encode().hex(), (s, e0, e1, line)


@pytest.mark.parametrize("build", ["plain", "san"])
def test_list_elements(programs, build):
    for (s, e0, e1), line in zip(CUTS, _run(programs[build], "L")):
        got = json.loads("[" + bytes.fromhex(line).decode() + "]")
        assert got == piece(s, e0, e1), (s, e0, e1, line)


@pytest.mark.parametrize("build", ["plain", "san"])
def test_entry_element(programs, build):
    for (s, e0, e1), line in zip(CUTS, _run(programs[build], "E")):
        got = json.loads("[" + bytes.fromhex(line).decode() + "]")
        assert got == piece(s, e0, e1)[-1:], (s, e0, e1, line)
