"""The encode record (crdt_amd/csrc/yc_encrec.h) on the CPU: tests/encrec_check.cpp built with the
address and undefined-behaviour sanitizers and run as a program. Pack -> unpack round-trips at header
lengths and tails of 0, 1, 2046 and 2047 (and every width between), 2048 is refused, every info
byte 0..255 survives, and the size read back from a record is 1 + header + (the varuint size of the
length of a deleted item | the content length of a live one).
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("encrec") / "encrec_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(HERE, "encrec_check.cpp")])
    return str(exe)


def test_record_round_trip_and_size(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    word, n = r.stdout.split()
    # edges x info bytes, every width 0..2048 both ways, 200 000 random records
    assert word == "ok" and int(n) == 10 * 10 * 5 * 2 * 256 + 2049 * 2 * 2 + 200000
