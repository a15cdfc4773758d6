"""yc_json.h any_json_text (lib0 `any` -> JSON.stringify text, the value writer of the fleet toJSON
kernels) against Node: tests/golden/any_json.json (tests/golden/gen/gen_any_json_fixtures.js) holds
hand-encoded and seeded `any` values with JSON.stringify of what Yjs 13.5.16 reads from them. The
host build of the function (tests/csrc/any_json_main.cpp) must give Node's text byte for byte, the
size-only pass must report exactly the bytes the write pass writes, the string sink of the host must
receive the bytes the device sink does, a value nested past the stack it is given (64 levels on the
device, 4000 on the host) and every truncated value must be refused. BigInt64 (JSON.stringify throws) is pinned against
Python's str(int). The same program is built a second time with AddressSanitizer and UBSan: inputs
and outputs sit in heap blocks of their exact size, so a read past a truncated value or a write
past the reported size aborts the run."""
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
AJ_OK, AJ_UNDEF, AJ_BAD, AJ_DEEP = 0, 1, 2, 3


def _fixture():
    with open(os.path.join(HERE, "golden", "any_json.json")) as f:
        return json.load(f)


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", *extra, "-I", os.path.join(ROOT, "crdt_amd", "csrc"),
                           os.path.join(HERE, "csrc", "any_json_main.cpp"), "-o", str(exe)])
    return exe


def _run(exe, fx):
    by_name = {c["name"]: c for c in fx["cases"]}
    lines = [f"V {c['any']}" for c in fx["cases"]]
    lines.append(f"V {fx['too_deep']}")
    lines += [f"T {by_name[n]['any']}" for n in fx["truncate"]]
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def _check(out, fx):
    cases = fx["cases"]
    for c, line in zip(cases, out):
        f = line.split(" ")
        assert f[0] == "V", (c["name"], line)
        status, sized, written, consumed = (int(x) for x in f[1:5])
        text = bytes.fromhex(f[5]) if len(f) > 5 else b""
        assert consumed == len(c["any"]) // 2, c["name"]
        if c.get("undef"):
            assert status == AJ_UNDEF and sized == 0 and written == 0, (c["name"], line)
            continue
        assert status == AJ_OK, (c["name"], line)
        assert sized == written == len(text), (c["name"], sized, written)
        want = str(int(c["big"])) if "big" in c else c["json"]
        assert text.decode("utf-8") == want, (c["name"], text, want)
    deep = out[len(cases)].split(" ")
    assert deep[0] == "V" and int(deep[1]) == AJ_DEEP, deep
    by_name = {c["name"]: c for c in cases}
    for n, line in zip(fx["truncate"], out[len(cases) + 1:]):
        f = line.split(" ")
        nbytes = len(by_name[n]["any"]) // 2
        assert f[0] == "T" and int(f[1]) == nbytes and int(f[2]) == nbytes, (n, line)  # every strict prefix refused


def _nest(n):
    """n containers, arrays and objects alternating, one member each, 0 at the bottom: (any as hex, text)"""
    enc = "".join("7501" if i % 2 == 0 else "7601016b" for i in range(n)) + "7d00"
    text = "".join("[" if i % 2 == 0 else '{"k":' for i in range(n)) + "0" + "".join("]" if i % 2 == 0 else "}" for i in reversed(range(n)))
    return enc, text


def _check_depths(exe):
    depths = (64, 65, 100, 2000, 4000, 4001)
    lines = [f"{m} {_nest(n)[0]}" for n in depths for m in "VH"]
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    out = [x.split(" ") for x in r.stdout.splitlines()]
    assert len(out) == len(lines)
    for k, n in enumerate(depths):
        enc, text = _nest(n)
        dev, host = out[2 * k], out[2 * k + 1]
        assert dev[0] == "V" and host[0] == "H", n
        if n <= 64:  # the 64-level stack
            assert int(dev[1]) == AJ_OK and int(dev[4]) == len(enc) // 2 and bytes.fromhex(dev[5]).decode() == text, n
        else:
            assert int(dev[1]) == AJ_DEEP, (n, dev[:2])
        if n <= 4000:  # the 4000-level stack
            assert int(host[1]) == AJ_OK and int(host[2]) == len(enc) // 2 and bytes.fromhex(host[3]).decode() == text, n
        else:
            assert int(host[1]) == AJ_DEEP, (n, host[:2])


def test_fixture_covers_the_forms():
    fx = _fixture()
    names = {c["name"] for c in fx["cases"]}
    for n in ("int_63", "int_64", "int_-64", "int_2147483647", "int_neg_zero", "f64_neg_zero", "f64_0.1+0.2", "f64_1e21",
              "f64_1e-7", "f64_5e-324", "f32_1.1", "nan", "inf", "ninf", "str_escapes", "str_ctl", "str_utf8", "obj_1",
              "arr_1", "obj_2", "arr_2", "arr_63", "mixed_63", "undef_in_obj", "undef_in_arr", "undef_top", "obj_empty",
              "arr_empty", "str_empty", "bin_0", "bin_3", "big_min"):
        assert n in names, n
    by = {c["name"]: c for c in fx["cases"]}
    assert by["f64_0.1+0.2"]["json"] == "0.30000000000000004" and by["f64_1e21"]["json"] == "1e+21"
    assert by["f64_5e-324"]["json"] == "5e-324" and by["f32_1.1"]["json"] == "1.100000023841858"
    assert by["nan"]["json"] == "null" and by["int_neg_zero"]["json"] == "0"
    assert by["undef_in_obj"]["json"] == '{"b":2}' and by["undef_in_arr"]["json"] == "[null,1,null]"
    assert by["bin_3"]["json"] == '{"0":0,"1":127,"2":255}' and by["undef_top"].get("undef")
    assert by["big_min"]["big"] == str(-2 ** 63)
    assert os.path.getsize(os.path.join(HERE, "golden", "any_json.json")) < 200_000


def test_any_json_text_matches_node(tmp_path):
    fx = _fixture()
    exe = _build(tmp_path, "any_json", [])
    _check(_run(exe, fx), fx)
    _check_depths(exe)


def test_any_json_text_sanitized(tmp_path):
    fx = _fixture()
    try:
        exe = _build(tmp_path, "any_json_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    except subprocess.CalledProcessError:
        pytest.fail("the sanitizer build of tests/csrc/any_json_main.cpp failed")
    _check(_run(exe, fx), fx)
    _check_depths(exe)


def test_docs_json_abi_without_a_device():
    """ycrdt_docs_json's argument checks and its n == 0 answer need no device."""
    import ctypes

    import crdt_amd

    L = crdt_amd.lib()
    assert "ycrdt_docs_json" in crdt_amd.EXPORTS and hasattr(L, "ycrdt_docs_json")
    out = crdt_amd._Out()
    offs = (ctypes.c_uint64 * 2)(7, 7)
    docs = (ctypes.c_void_p * 1)()
    roots = (ctypes.c_char_p * 1)(b"users")
    kinds = (ctypes.c_int * 1)(0)
    fake_engine = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))  # never dereferenced when n == 0
    E_ARG = -6
    assert L.ycrdt_docs_json(None, docs, roots, kinds, 0, ctypes.byref(out), offs, None) == E_ARG
    assert L.ycrdt_docs_json(fake_engine, None, roots, kinds, 0, ctypes.byref(out), offs, None) == E_ARG
    assert L.ycrdt_docs_json(fake_engine, docs, roots, kinds, 0, None, offs, None) == E_ARG
    assert L.ycrdt_docs_json(fake_engine, docs, roots, kinds, 0, ctypes.byref(out), None, None) == E_ARG
    assert L.ycrdt_docs_json(fake_engine, docs, None, kinds, 1, ctypes.byref(out), offs, None) == E_ARG
    assert L.ycrdt_docs_json(fake_engine, docs, roots, None, 1, ctypes.byref(out), offs, None) == E_ARG
    assert L.ycrdt_docs_json(fake_engine, docs, roots, kinds, 1, ctypes.byref(out), offs, None) == E_ARG  # a null doc
    st = crdt_amd.JsonStats()
    assert L.ycrdt_docs_json(fake_engine, docs, roots, kinds, 0, ctypes.byref(out), offs, ctypes.byref(st)) == 0
    assert offs[0] == 0 and out.len == 0
    assert st.pairs_device == st.pairs_single == st.pairs_empty == 0 and st.depth_max >= 4 and st.name_max >= 64
    L.ycrdt_free(ctypes.byref(out))
    with pytest.raises(ValueError):
        crdt_amd.docs_json([], ["x"], ["map"])
