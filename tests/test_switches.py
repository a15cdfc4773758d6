"""The environment switches (crdt_amd/csrc/yc_switches.h): one table, one reader.

tests/csrc/switches_main.cpp includes the header alone (no HIP), puts its arguments into the environment with
setenv, runs read_switches() and prints every field; the expected values below are written out by hand. The
program is built a second time with AddressSanitizer and UBSan (a stand-alone binary: nothing is loaded
into Python). The reader keeps the parsing every switch had at its point of use, quirks included: an off- or
on-switch looks at the FIRST character only, so "00" is off and "10" is on, while " 0", "" and "true" are
neither; keywords are compared as whole words; the integers go through atoi / strtoull (leading blanks skipped)
with the row's own range, and a value out of range is the default.

The second half compares the table with the sources and the documentation: no getenv outside the header, a
name's literal once in the C++ sources, the same names in INTEGRATION.md's table, and no test or script that
mentions a name the table does not have."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "crdt_amd", "csrc")

CAP = 1 << 31       # JSON_PASS_BYTES
SCHUNK = 1024       # SCHUNK (yc_common.h) = SCHUNK_LIMIT (asserted equal in yc_engine.hip)

# nothing set: every default, in the table's order
DEFAULT = (
    "decode=0 direct_wave=0 fwc=0 schunk=0 win_shift=32 pin_chunk=33554432 predecode=0 "
    "prewalk=1 walk_only=1 no_fastwalk=0 wdecode=0 spec_hint=2 fwm_max=0 fwc_walk=256 rtab=1 rank_last=1 "
    "test_section_cap=0 test_fail_before_exchange=0 decode_small=1 decode_quick=1 ds_grid=1 ds_jump=1 sd_group=1 "
    "scan_fused=1 debug_bounds=0 debug_yata=0 debug_decode=0 "
    "ds_tails=1 key_hash_bits=64 merge_small=1 phase_fence=0 yata_global=0 encode_small=1 enc_record=1 view_small=1 "
    "sync=1 store=1 docs_json=1 docs_cache=1 docs_read=1 docs_write=1 docs_transact=1 "
    "docs_json_pass_bytes=2147483648 docs_cache_pass_bytes=2147483648 docs_read_pass_bytes=2147483648 "
    "docs_write_pass_bytes=2147483648 docs_transact_pass_bytes=2147483648 "
    "debug_sync=0 rocprim_scan=0 yata=0 ylists_eager=0 view_sync=0 no_fold=0"
)

# (arguments, the fields that differ from DEFAULT)
CASES = [
    ([], {}),
    # off-switch: the first character '0'
    (["YCRDT_PREWALK=0"], {"prewalk": 0}),
    (["YCRDT_PREWALK=00"], {"prewalk": 0}),          # (first character only)
    (["YCRDT_PREWALK=0x"], {"prewalk": 0}),
    (["YCRDT_PREWALK=10"], {}),
    (["YCRDT_PREWALK=1"], {}),
    (["YCRDT_PREWALK=true"], {}),
    (["YCRDT_PREWALK=false"], {}),
    (["YCRDT_PREWALK"], {}),                         # the empty string
    (["YCRDT_PREWALK= 0"], {}),
    # on-switch: the first character '1'
    (["YCRDT_PHASE_FENCE=1"], {"phase_fence": 1}),
    (["YCRDT_PHASE_FENCE=10"], {"phase_fence": 1}),  # (first character only)
    (["YCRDT_PHASE_FENCE=00"], {}),
    (["YCRDT_PHASE_FENCE=0"], {}),
    (["YCRDT_PHASE_FENCE=true"], {}),
    (["YCRDT_PHASE_FENCE"], {}),
    (["YCRDT_PHASE_FENCE= 1"], {}),
    # set at all
    (["YCRDT_YATA_GLOBAL=0"], {"yata_global": 1}),
    (["YCRDT_YATA_GLOBAL"], {"yata_global": 1}),
    (["YCRDT_YATA_GLOBAL=1"], {"yata_global": 1}),
    # keywords: whole words (decode: 1 chunks, 2 direct, 3 xtab)
    (["YCRDT_DECODE=chunks"], {"decode": 1}),
    (["YCRDT_DECODE=tables"], {"decode": 1}),
    (["YCRDT_DECODE=direct"], {"decode": 2}),
    (["YCRDT_DECODE=xtab"], {"decode": 3}),
    (["YCRDT_DECODE=chunk"], {}),                    # a typo forces nothing
    (["YCRDT_DECODE=chunks "], {}),
    (["YCRDT_DECODE=CHUNKS"], {}),
    (["YCRDT_DECODE=00"], {}),
    (["YCRDT_DECODE=10"], {}),
    (["YCRDT_DECODE=true"], {}),
    (["YCRDT_DECODE"], {}),
    (["YCRDT_DECODE= 0"], {}),
    (["YCRDT_YATA=seq"], {"yata": 1}),
    (["YCRDT_YATA=seq "], {}),
    (["YCRDT_YATA=1"], {}),
    (["YCRDT_WDECODE=settle"], {"wdecode": 1}),
    (["YCRDT_WDECODE=settled"], {}),
    # ... and a first character beside them (fwc: 1 off, 2 force; predecode: 1 off, 2 check; direct_wave: 1 lane, 2 wave)
    (["YCRDT_FWC=0"], {"fwc": 1}),
    (["YCRDT_FWC=00"], {"fwc": 1}),
    (["YCRDT_FWC=force"], {"fwc": 2}),
    (["YCRDT_FWC=forced"], {}),
    (["YCRDT_FWC=1"], {}),
    (["YCRDT_FWC"], {}),
    (["YCRDT_PREDECODE=0"], {"predecode": 1}),
    (["YCRDT_PREDECODE=check"], {"predecode": 2}),
    (["YCRDT_PREDECODE=checks"], {}),
    (["YCRDT_PREDECODE=1"], {}),
    (["YCRDT_DIRECT_WAVE=0"], {"direct_wave": 1}),
    (["YCRDT_DIRECT_WAVE=1"], {"direct_wave": 2}),
    (["YCRDT_DIRECT_WAVE=2"], {}),
    (["YCRDT_DIRECT_WAVE= 0"], {}),
    (["YCRDT_SPEC_HINT=1"], {"spec_hint": 1}),
    (["YCRDT_SPEC_HINT=0"], {"spec_hint": 0}),
    (["YCRDT_SPEC_HINT=2"], {}),
    (["YCRDT_SPEC_HINT"], {}),
    # bounded integers
    (["YCRDT_SCHUNK=63"], {}),
    (["YCRDT_SCHUNK=64"], {"schunk": 64}),
    (["YCRDT_SCHUNK=96"], {}),                       # no multiple of 64
    (["YCRDT_SCHUNK=128"], {"schunk": 128}),
    ([f"YCRDT_SCHUNK={SCHUNK}"], {"schunk": SCHUNK}),
    ([f"YCRDT_SCHUNK={SCHUNK + 64}"], {}),
    (["YCRDT_SCHUNK=00"], {}),
    (["YCRDT_SCHUNK=10"], {}),
    (["YCRDT_SCHUNK=true"], {}),
    (["YCRDT_SCHUNK"], {}),
    (["YCRDT_SCHUNK= 0"], {}),
    (["YCRDT_SCHUNK=-64"], {}),
    (["YCRDT_WIN_SHIFT=15"], {}),
    (["YCRDT_WIN_SHIFT=16"], {"win_shift": 16}),
    (["YCRDT_WIN_SHIFT=32"], {}),
    (["YCRDT_WIN_SHIFT=33"], {}),
    (["YCRDT_WIN_SHIFT= 16"], {"win_shift": 16}),    # (atoi skips the blank)
    (["YCRDT_FWM_MAX=0"], {}),                       # unset and 0: no limit
    (["YCRDT_FWM_MAX=5"], {"fwm_max": 5}),
    (["YCRDT_KEY_HASH_BITS=0"], {}),                 # unset and 0: all 64 bits
    (["YCRDT_KEY_HASH_BITS=4"], {"key_hash_bits": 4}),
    (["YCRDT_KEY_HASH_BITS=63"], {"key_hash_bits": 63}),
    (["YCRDT_KEY_HASH_BITS=64"], {}),
    (["YCRDT_KEY_HASH_BITS=-1"], {}),
    (["YCRDT_TEST_SECTION_CAP=0"], {}),
    (["YCRDT_TEST_SECTION_CAP=-3"], {}),
    (["YCRDT_TEST_SECTION_CAP=7"], {"test_section_cap": 7}),
    (["YCRDT_FWC_WALK=0"], {}),
    (["YCRDT_FWC_WALK=9"], {"fwc_walk": 9}),
    (["YCRDT_PIN_CHUNK=4095"], {}),
    (["YCRDT_PIN_CHUNK=4096"], {"pin_chunk": 4096}),
    (["YCRDT_PIN_CHUNK=65536"], {"pin_chunk": 65536}),
    ([f"YCRDT_PIN_CHUNK={1 << 30}"], {"pin_chunk": 1 << 30}),
    ([f"YCRDT_PIN_CHUNK={(1 << 30) + 1}"], {}),
    (["YCRDT_PIN_CHUNK=words"], {}),
    # the bytes of a pass: pass_bytes (tests/test_engine_host.py), each call its own variable
    (["YCRDT_DOCS_JSON_PASS_BYTES=600"], {"docs_json_pass_bytes": 600}),
    (["YCRDT_DOCS_CACHE_PASS_BYTES=601"], {"docs_cache_pass_bytes": 601}),
    (["YCRDT_DOCS_READ_PASS_BYTES=602"], {"docs_read_pass_bytes": 602}),
    (["YCRDT_DOCS_WRITE_PASS_BYTES=603"], {"docs_write_pass_bytes": 603}),
    (["YCRDT_DOCS_TRANSACT_PASS_BYTES=604"], {"docs_transact_pass_bytes": 604}),
    (["YCRDT_DOCS_JSON_PASS_BYTES=0"], {}),
    ([f"YCRDT_DOCS_JSON_PASS_BYTES={CAP + 1}"], {}),
    # a value of 4 096 characters (nothing copies it into a fixed buffer)
    (["YCRDT_PREWALK=@4096"], {"prewalk": 0}),
    (["YCRDT_PHASE_FENCE=@4096"], {}),
    (["YCRDT_DECODE=@4096"], {}),
    (["YCRDT_YATA_GLOBAL=@4096"], {"yata_global": 1}),
    (["YCRDT_SCHUNK=@4093+128"], {"schunk": 128}),
    (["YCRDT_DOCS_READ_PASS_BYTES=@4093+700"], {"docs_read_pass_bytes": 700}),
    # several at once, every other off- and on-switch once
    (["YCRDT_DECODE=direct", "YCRDT_DIRECT_WAVE=0", "YCRDT_MERGE_SMALL=0", "YCRDT_DEBUG_BOUNDS=1"],
     {"decode": 2, "direct_wave": 1, "merge_small": 0, "debug_bounds": 1}),
    (["YCRDT_WALK_ONLY=0", "YCRDT_RTAB=0", "YCRDT_RANK_LAST=0", "YCRDT_DECODE_SMALL=0", "YCRDT_DECODE_QUICK=0", "YCRDT_DS_GRID=0",
      "YCRDT_DS_JUMP=0", "YCRDT_SD_GROUP=0", "YCRDT_SCAN_FUSED=0", "YCRDT_DS_TAILS=0", "YCRDT_ENCODE_SMALL=0", "YCRDT_ENC_RECORD=0",
      "YCRDT_VIEW_SMALL=0", "YCRDT_SYNC=0", "YCRDT_STORE=0", "YCRDT_DOCS_JSON=0", "YCRDT_DOCS_CACHE=0", "YCRDT_DOCS_READ=0",
      "YCRDT_DOCS_WRITE=0", "YCRDT_DOCS_TRANSACT=0"],
     {"walk_only": 0, "rtab": 0, "rank_last": 0, "decode_small": 0, "decode_quick": 0, "ds_grid": 0, "ds_jump": 0, "sd_group": 0,
      "scan_fused": 0, "ds_tails": 0, "encode_small": 0, "enc_record": 0, "view_small": 0, "sync": 0, "store": 0, "docs_json": 0,
      "docs_cache": 0, "docs_read": 0, "docs_write": 0, "docs_transact": 0}),
    (["YCRDT_NO_FASTWALK=1", "YCRDT_TEST_FAIL_BEFORE_EXCHANGE=1", "YCRDT_DEBUG_YATA=1", "YCRDT_DEBUG_DECODE=1", "YCRDT_DEBUG_SYNC=1",
      "YCRDT_ROCPRIM_SCAN=1", "YCRDT_YLISTS_EAGER=1", "YCRDT_VIEW_SYNC=1", "YCRDT_NO_FOLD=1"],
     {"no_fastwalk": 1, "test_fail_before_exchange": 1, "debug_yata": 1, "debug_decode": 1, "debug_sync": 1, "rocprim_scan": 1,
      "ylists_eager": 1, "view_sync": 1, "no_fold": 1}),
]


def _want(diff):
    fields = [f.split("=") for f in DEFAULT.split()]
    assert set(diff) <= {k for k, _ in fields}, diff
    return " ".join(f"{k}={diff.get(k, v)}" for k, v in fields)


def _build(tmp_path, name, extra):
    exe = os.path.join(str(tmp_path), name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-I", CSRC,
                           os.path.join(HERE, "csrc", "switches_main.cpp"), "-o", exe])
    return exe


def _check(exe):
    env = {k: v for k, v in os.environ.items() if not k.startswith("YCRDT_")}
    for args, diff in CASES:
        r = subprocess.run([exe, *args], capture_output=True, text=True, env=env)
        assert r.returncode == 0, (args, r.stdout[-1000:], r.stderr[-3000:])
        assert r.stdout == _want(diff) + "\n", args


def test_switches_parse(tmp_path):
    _check(_build(tmp_path, "switches", []))


def test_switches_parse_sanitized(tmp_path):
    try:
        exe = _build(tmp_path, "switches_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    except subprocess.CalledProcessError:
        pytest.fail("the sanitizer build of tests/csrc/switches_main.cpp failed")
    _check(exe)


# ---- the table against the sources and the documentation
NAME = re.compile(r"YCRDT_[A-Z0-9_]+")
# read outside the C++ library: the Node addon (crdt_amd/js/ycrdt_napi.c), the host hub, the Python binding, bench.py
OUTSIDE = {"YCRDT_COMPAT", "YCRDT_HUB_TOKEN", "YCRDT_HUB_MAX_FRAME", "YCRDT_HUB_PORT", "YCRDT_LIB", "YCRDT_DEVICE"}
# include/ycrdt.h's return codes: names of the same shape that are no switches
CODES = {"YCRDT_OK", "YCRDT_E_DECODE", "YCRDT_E_PENDING", "YCRDT_E_UNSUPPORTED", "YCRDT_E_CAPACITY", "YCRDT_E_DEVICE", "YCRDT_E_ARG"}


def _sources():
    return {f: open(os.path.join(CSRC, f), encoding="utf-8").read() for f in sorted(os.listdir(CSRC))
            if f.endswith((".h", ".hip", ".cpp"))}


def _table():
    rows = re.findall(r'^  X\([\w:]+, (\w+), "(YCRDT_[A-Z0-9_]+)", \w+, [^"]+, (PROCESS|ENGINE|BATCH|CALL), "', _sources()["yc_switches.h"], re.M)
    assert len(rows) == len(DEFAULT.split()) and [f for f, _, _ in rows] == [f.split("=")[0] for f in DEFAULT.split()]
    return {name: when for _, name, when in rows}


def _documented():
    text = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    section = text.split("## Environment switches", 1)[1].split("\n## ", 1)[0]
    return [ln for ln in section.splitlines() if ln.startswith("| `YCRDT_")]


def test_getenv_only_in_the_table():
    for f, text in _sources().items():
        if f != "yc_switches.h":
            assert "getenv(" not in text, f


def test_every_name_once_in_the_sources():
    literals = [m for text in _sources().values() for m in re.findall(r'"(YCRDT_[A-Z0-9_]+)"', text)]
    assert sorted(literals) == sorted(_table())


def test_documentation_lists_the_table():
    table = _table()
    rows = _documented()
    cut = re.compile(r"(?<!\\)\|")  # (a cell may hold an escaped bar)
    names = [n for ln in rows for n in NAME.findall(cut.split(ln)[1])]
    assert len(names) == len(set(names)), "a switch documented twice"
    assert set(names) - OUTSIDE == set(table)
    assert OUTSIDE <= set(names)
    when = {"PROCESS": "process", "ENGINE": "engine", "BATCH": "batch", "CALL": "call"}
    for ln in rows:  # | names | read | default | effect |
        cells = [c.strip() for c in cut.split(ln)]
        for n in NAME.findall(cells[1]):
            if n in table:
                assert cells[2].split(",")[0].split(" ")[0] == when[table[n]], n


def test_tests_and_scripts_name_known_switches():
    known = set(_table()) | OUTSIDE | CODES
    for top in ("tests", "scripts"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if not f.endswith((".py", ".js", ".mjs", ".sh", ".c", ".cpp", ".h")):
                    continue
                text = open(os.path.join(d, f), encoding="utf-8", errors="replace").read()
                unknown = set(NAME.findall(text)) - known
                assert not unknown, (os.path.join(d, f), sorted(unknown))
