"""yc_read.h on the host: the comparator of the order the fleet toJSON radix passes leave the view
keys in — (container, name bytes zero-padded to 64 big-endian, name length) — and the search for one
entry name in one container, which the point-read kernels (yc_read.hip, ycrdt_docs_read) run one
lane per read. tests/csrc/read_order_main.cpp sorts the names by the passes themselves, then checks
that the comparator agrees with that order, that every name is found at its own position and that
absent names are not found, under AddressSanitizer and UBSan with every name in a heap block of its
exact size. The names are those of test_entry_order_and_long_name (tests/test_gpu_docs_json.py)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

P8, P16, P40 = b"01234567", b"0123456789abcdef", b"z" * 40
NAMES = list(dict.fromkeys([
    P8 + b"B", P8 + b"A", P8, P16 + b"\xc3\xa9", P16 + b"e", P16, P40 + b"2", P40 + b"10", P40, b"a", b"a\x00", b"a\x00\x00",
    b"", b"\xf0\x9f\x98\x80", b"\xc3\xbf", b"\x7f", b"b" * 64, b"b" * 63 + b"a", b"b" * 63]))
ABSENT = [
    P8 + b"C", P8 + b"\x00", P8[:7], P8[:7] + b"8", P16 + b"\xc3", P16 + b"\xc3\xaa", P16 + b"f", P16[:15], P40 + b"1", P40 + b"11",
    P40 + b"3", P40[:39], b"a\x00\x00\x00", b"a\x01", b"\x00", b"\xf0\x9f\x98", b"\xf0\x9f\x98\x81", b"\xc3", b"b" * 62,
    b"b" * 63 + b"b" + b""[:0] + b"", b"c" * 64, b"\x7e"]
ABSENT = [n for n in dict.fromkeys(ABSENT) if n not in NAMES]


def _build(tmp_path):
    exe = tmp_path / "read_order"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "crdt_amd", "csrc"), os.path.join(HERE, "csrc", "read_order_main.cpp"), "-o", str(exe)])
    return exe


def _run(exe, lines):
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    out = r.stdout.splitlines()
    assert out[-1].startswith("OK ") and not any(x.startswith("FAIL") for x in out), out
    return out


def _line(kind, group, name):
    return f"{kind} {group} {name.hex() or '-'}"


def test_names_found_at_their_own_position_and_absent_ones_not(tmp_path):
    assert len(ABSENT) >= 20
    exe = _build(tmp_path)
    # the same names in two containers (a nested type's unit and a root key), and one container holding one name only
    groups = (7, (1 << 63) | (3 << 32) | 12345)
    lines = [_line("P", g, n) for g in groups for n in NAMES] + [_line("P", 9, b"a")]
    lines += [_line("A", g, n) for g in groups for n in ABSENT] + [_line("A", 9, n) for n in NAMES if n != b"a"] + [_line("A", 8, b"a")]
    out = _run(exe, lines)
    answers = [x.split() for x in out[:-1]]
    assert len(answers) == len(lines)
    assert all(a[2] != "none" and a[3] == "0" for a in answers if a[0] == "P")
    assert all(a[2] == "none" and a[3] == "0" for a in answers if a[0] == "A")
    # positions inside one container ascend with the name bytes, a prefix first
    pos = {bytes.fromhex(l.split()[2].replace("-", "")): int(a[2]) for l, a in zip(lines, answers) if l.startswith("P 7 ")}
    assert [n for n, _ in sorted(pos.items(), key=lambda kv: kv[1])] == sorted(NAMES)


def test_a_name_past_the_bound_makes_its_prefix_ambiguous(tmp_path):
    exe = _build(tmp_path)
    long_name = b"b" * 64 + b"L" * 236
    lines = [_line("P", 7, n) for n in NAMES] + [_line("L", 7, long_name), _line("A", 7, b"b" * 62), _line("P", 8, b"b" * 64)]
    out = _run(exe, lines)
    amb = {l: a.split()[3] for l, a in zip(lines, out[:-1])}
    assert amb[_line("P", 7, b"b" * 64)] == "1" and amb[_line("L", 7, long_name)] == "1"
    assert amb[_line("P", 7, b"b" * 63)] == "0" and amb[_line("P", 7, b"b" * 63 + b"a")] == "0"
    assert amb[_line("P", 8, b"b" * 64)] == "0"  # another container
    assert sum(v == "1" for v in amb.values()) == 2
