"""yc_cache.h on the host: index_kind (JavaScript's `val == 'map'` over an index entry's content
bytes) against what Yjs 13.5.16 and Node did with every index entry of tests/golden/cache.json
(Array.isArray(c[name])), and cache_put_name (a member's `"name":`) against Node's
JSON.stringify(name). tests/csrc/index_kind_main.cpp is built plain and with AddressSanitizer and
UBSan: every input sits in a heap block of its exact size, so a read past a truncated or overlong
value aborts the run. The hand-made encodings pin what lib0's readers do with them: an overlong
varuint is read as its value, a seventh varuint byte or a value that ends early is no 'map'."""
import os
import subprocess

import pytest

from tests.cache_fixture import cases, element_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

MAP = "77036d6170"  # the `any` string "map"


def _json(text):  # ContentJSON / ContentEmbed: length, JSON text
    b = text.encode()
    assert len(b) < 128
    return bytes([len(b)]).hex() + b.hex()


# (content ref, hex, index_kind)
HAND = [
    (8, MAP, 1),
    (8, MAP + "ff", 1),                       # only the first value is read
    (8, "7501" + MAP, 1),
    (8, "7501" * 1000 + MAP, 1),              # no depth limit: nothing is kept per level
    (8, "7501" * 1000, 0),
    (8, "7502" + MAP + MAP, 0),
    (8, "7500", 0),
    (8, "778300" + "6d6170", 1),              # length 3 written overlong
    (8, "758100" + MAP, 1),                   # count 1 written overlong
    (8, "77838080808000" + "6d6170", 1),      # ... in six bytes, the most lib0 0.2.42 reads
    (8, "7783808080808000" + "6d6170", 0),    # a seventh varuint byte
    (8, "7583", 0),
    (8, "77036d61", 0),                       # the string ends early
    (8, "77046d617000", 0),
    (8, "77034d6170", 0),
    (8, "7f", 0), (8, "7e", 0), (8, "7d01", 0), (8, "7600", 0), (8, "74036d6170", 0), (8, "", 0), (8, "00", 0),
    (3, "036d6170", 0),                       # ContentBinary
    (4, "6d6170", 0),                         # ContentString: an entry's value is one character
    (7, "01", 0), (7, "00", 0),               # a shared type
    (2, _json('"map"'), 1), (2, _json('["map"]'), 1), (2, _json(' [ [\t"map" ]\n] '), 1), (5, _json('"map"'), 1),
    (2, _json('"Map"'), 0), (2, _json('["map"'), 0), (2, _json('"map"]'), 0), (2, _json('"map'), 0), (2, _json('map'), 0),
    (2, _json('["map","map"]'), 0), (2, _json('{}'), 0), (2, "05" + b'"ma'.hex(), 0), (2, "", 0), (2, "00", 0),
]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("index_kind")
    out = {}
    for name, extra in (("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = d / name
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", *extra, "-I", os.path.join(ROOT, "crdt_amd", "csrc"),
                               os.path.join(HERE, "csrc", "index_kind_main.cpp"), "-o", str(exe)])
        out[name] = exe
    return out


def _run(exe, lines):
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


@pytest.mark.parametrize("build", ["plain", "san"])
def test_index_kind_fixture(programs, build):
    entries = [(c["name"], e) for c in cases() for e in c["entries"]]
    assert len(entries) >= 90
    out = _run(programs[build], [f"K {e['ref']} {element_bytes(e).hex()}" for _, e in entries])
    for (cname, e), line in zip(entries, out):
        assert line == f"K {0 if e['is_array'] else 1}", (cname, e["name"], e["content"], line)


@pytest.mark.parametrize("build", ["plain", "san"])
def test_index_kind_hand_made(programs, build):
    out = _run(programs[build], [f"K {ref} {h}" for ref, h, _ in HAND])
    for (ref, h, want), line in zip(HAND, out):
        assert line == f"K {want}", (ref, h[:40], line)
    # every strict prefix of a value that is 'map' is not
    for ref, h, want in HAND:
        if want and len(h) < 200:
            pre = [h[:2 * k] for k in range(len(h) // 2)]
            if h.endswith("ff"):
                pre = pre[:-1]  # (without the trailing byte the value is whole)
            for p, line in zip(pre, _run(programs[build], [f"K {ref} {p}" for p in pre])):
                assert line == "K 0", (ref, p)


@pytest.mark.parametrize("build", ["plain", "san"])
def test_name_prefix(programs, build):
    names = {e["name"]: e["name_json"] for c in cases() for e in c["entries"]}
    assert {"", "\"", "\\", "\x01", " ", "\U0001F600"} <= set(names)
    keys = list(names)
    out = _run(programs[build], [f"N {k.encode().hex()}" for k in keys])
    for k, line in zip(keys, out):
        f = line.split(" ")
        text = bytes.fromhex(f[2])
        assert f[0] == "N" and int(f[1]) == len(text), (k, line)
        assert text.decode() == names[k] + ":", (k, text)
