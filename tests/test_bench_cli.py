"""bench.py's command line: a plain run times the headline only, --full adds the side legs, and
--dump-outputs writes the last timed merge's results as float .npy arrays that two runs with the
same arguments reproduce."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE_LEGS = ("single_doc", "end_to_end", "cpu_baseline", "fleet_sync", "fleet_ingest", "apply_loop",
             "full_state_ingest", "per_op", "c3", "c4", "c4_sharded", "fleet_ranks", "billion")


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench

    return bench


def test_dump_small_outputs_are_whole(tmp_path):
    bench = _bench()
    res = [(bytes(range(40)), b"\x01\x05\x07"), (b"\xff" * 9, b"\x00")]
    bench.dump_outputs(str(tmp_path), res, 0, 1)
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sorted(got) == ["state_vectors", "sv_crc32", "sv_lengths", "update_crc32", "update_lengths", "updates"]
    assert got["updates"].dtype == np.float32 and got["update_lengths"].dtype == np.float64
    assert got["updates"].tolist() == list(range(40)) + [255.0] * 9
    assert got["state_vectors"].tolist() == [1.0, 5.0, 7.0, 0.0]
    assert got["update_lengths"].tolist() == [40.0, 9.0] and got["sv_lengths"].tolist() == [3.0, 1.0]
    assert got["update_crc32"].tolist() == [float(zlib.crc32(u)) for u, _ in res]


def test_dump_sample_is_bounded_and_fixed(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_UPDATE_BYTES", 1000)
    rng = np.random.default_rng(3)
    res = [(rng.integers(0, 256, 5000 + 17 * i, dtype=np.uint8).tobytes(), b"\x00") for i in range(7)]
    res.append((b"\x09" * 100, b"\x00"))  # shorter than its share: kept whole
    bench.dump_outputs(str(tmp_path / "a"), res, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), res, 0, 1)
    a, b = np.load(tmp_path / "a" / "updates.npy"), np.load(tmp_path / "b" / "updates.npy")
    assert a.size == 7 * (1000 // 8) + 100 and np.array_equal(a, b)
    assert a[-100:].tolist() == [9.0] * 100
    other = list(res)
    other[2] = (bytes(len(res[2][0])), b"\x00")  # one document's bytes change: its checksum and sample do
    bench.dump_outputs(str(tmp_path / "c"), other, 0, 1)
    c = np.load(tmp_path / "c" / "updates.npy")
    k = 1000 // 8
    assert np.array_equal(a[:2 * k], c[:2 * k]) and np.array_equal(a[3 * k:], c[3 * k:]) and not c[2 * k:3 * k].any()
    assert np.load(tmp_path / "c" / "update_crc32.npy")[2] != np.load(tmp_path / "a" / "update_crc32.npy")[2]
    # more than one rank: every rank's files carry its number
    bench.dump_outputs(str(tmp_path / "r"), res, 1, 2)
    assert "updates_rank1.npy" in os.listdir(tmp_path / "r")


def test_full_is_off_by_default(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert not a.full and a.dump_outputs is None and a.steps == 7
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "x"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "x"


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    """A small plain run (3 documents of 8 replicas): the timed steps are the ones asked for, no side
    leg ran, and the dumped arrays are the merge of the same documents through Batch."""
    import crdt_amd
    from crdt_amd.workload import C2, gen_map

    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--docs", "3", "--replicas", "8", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False and d["ms_per_step"] > 0
    assert d["unit"] == "items/s" and d["higher_is_better"] is True
    assert d["value"] == pytest.approx(d["config"]["items_per_step_per_gpu"] / (d["ms_per_step"] * 1e-3), rel=1e-3)
    assert all(d[k] is None for k in SIDE_LEGS)
    assert d["roofline"]["kernels"]
    cfg = dict(C2, n_replicas=8)
    docs = [gen_map(**dict(cfg, seed=C2["seed"] + i * 1_009))[0] for i in range(3)]
    want = crdt_amd.merge_docs(docs)
    ups = np.load(out / "updates.npy")
    svs = np.load(out / "state_vectors.npy")
    assert ups.dtype == np.float32 and svs.dtype == np.float32
    assert ups.astype(np.uint8).tobytes() == b"".join(u for u, _ in want)
    assert svs.astype(np.uint8).tobytes() == b"".join(v for _, v in want)
    assert np.load(out / "update_lengths.npy").tolist() == [float(len(u)) for u, _ in want]
    assert np.load(out / "update_crc32.npy").tolist() == [float(zlib.crc32(u)) for u, _ in want]
    assert sum(len(u) + len(v) for u, v in want) == d["config"]["output_bytes"]
