"""The struct decode's shape classifier (crdt_amd/csrc/yc_shape.h) on the CPU: tests/shape_check.cpp
built with the address and undefined-behaviour sanitizers and run as a program. Over random windows
and over the first bytes of every struct of the golden fixtures the class is below NCLASS and no byte
outside the 24-byte window is read; over hand-built structs of known kinds the class is the one the
kind should get (a wrong class only costs time, but the sort is worth nothing if the classes are off).
"""
import json
import os
import shutil
import subprocess

import pytest

from oracle import ymerge
from tests.struct_shapes import KINDS, Builder

HERE = os.path.dirname(os.path.abspath(__file__))
NCLASS = 13
# kind (tests/struct_shapes.py) -> class (yc_shape.h)
CLASS_OF = {"deleted": 1, "int": 2, "string": 3, "object": 4, "array": 4, "root_key": 8, "root_id": 11, "gc": 0, "skip": 0,
            "cstring": 3, "binary": 3, "type": 5, "embed": 5, "format": 5, "json": 5, "rorigin": 6, "other": 12,
            "nested_any": 4, "doc": 5}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("shape") / "shape_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(HERE, "shape_check.cpp")])
    return str(exe)


def _run(checker, tmp_path, records):
    path = tmp_path / "records.bin"
    path.write_bytes(b"".join(records))
    r = subprocess.run([checker, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    classes = [int(x) for x in r.stdout.split()]
    assert len(classes) == len(records)
    return classes


def _record(update, p):
    s = p & ~3
    return (update[s:s + 24] + bytes(24))[:24] + bytes([p & 3])


def _struct_starts(update):
    """Byte offset of every struct of a valid update (the walk of ymerge.lazy_structs)."""
    d = ymerge.Dec(update)
    out = []
    for _ in range(d.vu()):
        n = d.vu()
        d.vu()
        d.vu()
        for _ in range(n):
            out.append(d.p)
            info = d.u8()
            if info & 31 in (0, 10):
                d.vu()
                continue
            for _ in range(2 * bin(info & 0xC0).count("1")):
                d.vu()
            if info & 0xC0 == 0:
                if d.vu() == 1:
                    d.vstr_raw()
                else:
                    d.vu()
                    d.vu()
                if info & 0x20:
                    d.vstr_raw()
            ymerge.read_content(d, info)
    return out


def test_random_windows(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    hist = dict(line.replace("class ", "").split(": ") for line in r.stdout.strip().splitlines())
    assert len(hist) == NCLASS and sum(int(v) for v in hist.values()) == 400000
    assert sum(1 for v in hist.values() if int(v) > 0) >= NCLASS - 1  # the noise reaches the classes


def test_golden_fixture_structs(checker, tmp_path):
    records = []
    for name in ("configs.json", "map.json", "array.json", "nested.json"):
        with open(os.path.join(HERE, "golden", name)) as f:
            fx = json.load(f)
        cases = fx["cases"] if isinstance(fx, dict) else fx
        for c in cases:
            for u in c["updates"]:
                u = bytes.fromhex(u)
                records += [_record(u, p) for p in _struct_starts(u)]
    assert len(records) > 1000
    classes = _run(checker, tmp_path, records)
    assert max(classes) < NCLASS
    # the fixtures' structs are the common shapes: few fall out of the window
    assert sum(1 for c in classes if c == NCLASS - 1) < len(classes) // 10


def test_hand_built_kinds(checker, tmp_path):
    b = Builder(7, "k")
    for k in range(400):
        b.add((KINDS + ("other", "nested_any", "doc"))[k % (len(KINDS) + 3)], lazy=True)
    u = b.update()
    assert _struct_starts(u) == [p for p, _ in b.starts()]
    starts = b.starts()
    classes = _run(checker, tmp_path, [_record(u, p) for p, _ in starts])
    seen = set()
    for k, ((p, kind), cls) in enumerate(zip(starts, classes)):
        want = CLASS_OF[kind]
        if u[p] & 0xC0 == 0 and u[p] & 31 not in (0, 10) and kind not in ("root_key", "root_id", "other"):
            want = 8 if want <= 2 else 9 if want == 3 else 10  # the list's first item, the nested type: root headers
        assert cls == want, (k, kind, cls, want)
        seen.add(kind)
    assert seen >= set(CLASS_OF)
    # a large client id (5-byte varuints) keeps the common item inside the window
    b = Builder(0x7FFFFFF1, "k")
    for k in range(3000):
        b.add(KINDS[k % 5])
    u = b.update()
    classes = _run(checker, tmp_path, [_record(u, p) for p, _ in b.starts()])
    assert all(c == CLASS_OF[kind] for (_, kind), c in list(zip(b.starts(), classes))[1:])
