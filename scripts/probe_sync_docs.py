#!/usr/bin/env python3
"""Probe of the batched sync responder (ycrdt_docs_diff): three shapes, each timed three ways.

Shapes
  c2_lagging   one C2-shaped document (crdt_amd.workload.C2), 256 peers each lagging by the last
               few ops of a few clients;
  c2_joiners   the same document, 16 fresh joiners (empty state vector: the full state);
  c5_fleet     10 000 small documents (the Yjs-generated C5 fixtures, cycled) merged by
               apply_updates_multi — no marks — with one lagging peer each.
Ways
  docs_diff    the new path, with its phase times (one profiled call);
  single       the same call with YCRDT_SYNC=0: every pair through ycrdt_encode_state_as_update —
               the path a responder had before, the baseline of the ratios;
  packed_diff  states_packed + diff_updates (Y.diffUpdate bytes: not the same reply; for scale).

Times are host wall clock around calls that end in the device-to-host copy, after warm-up calls of
the same shape; median and minimum over the repeats. Prints one JSON line.

  python scripts/probe_sync_docs.py [--scale 1.0] [--repeats 7] [--out FILE]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import crdt_amd  # noqa: E402
from crdt_amd import workload  # noqa: E402


def vu(v):
    out = bytearray()
    while v > 127:
        out.append(0x80 | (v & 0x7F))
        v >>= 7
    out.append(v)
    return bytes(out)


def read_sv(b):
    p, vals = 0, []

    def rd():
        nonlocal p
        v, s = 0, 0
        while True:
            x = b[p]
            p += 1
            v |= (x & 0x7F) << s
            s += 7
            if x < 0x80:
                return v

    for _ in range(rd()):
        vals.append((rd(), rd()))
    return vals


def write_sv(entries):
    return vu(len(entries)) + b"".join(vu(c) + vu(k) for c, k in entries)


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "repeats": repeats}


def measure(eng, docs, svs, unique_docs, state_max, warmup, repeats):
    out = {"pairs": len(docs), "docs": len(unique_docs)}
    new, st = crdt_amd.docs_diff_stats(docs, svs, engine=eng)
    out["stats"] = st
    out["reply_bytes"] = sum(len(r) for r in new)
    out["docs_diff"] = timed(lambda: crdt_amd.docs_diff(docs, svs, engine=eng), warmup, repeats)
    eng.set_profiling(True)
    crdt_amd.docs_diff(docs, svs, engine=eng)
    out["docs_diff"]["phases_ms"] = {k: round(v, 4) for k, v in eng.phase_times()}
    eng.set_profiling(False)
    os.environ["YCRDT_SYNC"] = "0"
    try:
        old, st0 = crdt_amd.docs_diff_stats(docs, svs, engine=eng)
        assert st0["pairs_single"] == len(docs)
        out["single"] = timed(lambda: crdt_amd.docs_diff(docs, svs, engine=eng), 1, max(3, repeats // 2))
    finally:
        del os.environ["YCRDT_SYNC"]
    out["identical"] = new == old
    # states_packed + diff_updates stages every pair's whole state again: at most 256 MB of it per call
    # (compared per pair). The pairs' documents are unique_docs[0] for all, or unique_docs[i] for pair i.
    k = max(1, min(len(docs), (256 << 20) // max(1, state_max)))
    kdocs, ksvs = docs[:k], [sv if sv else b"\x00" for sv in svs[:k]]
    kuniq = unique_docs if len(unique_docs) == 1 else unique_docs[:k]

    def packed_diff():
        blob, offs = crdt_amd.states_packed(kuniq, engine=eng)
        o = offs.tolist()
        states = [bytes(blob[o[2 * i]:o[2 * i + 1]]) for i in range(len(kuniq))]
        pos = {id(d): i for i, d in enumerate(kuniq)}
        return crdt_amd.diff_updates([states[pos[id(d)]] for d in kdocs], ksvs, engine=eng)

    out["packed_diff"] = timed(packed_diff, 1, max(3, repeats // 2))
    out["packed_diff"]["pairs"] = k
    per = lambda key, n: out[key]["median_ms"] / n  # noqa: E731
    out["ratio_single_over_docs_diff"] = round(out["single"]["median_ms"] / out["docs_diff"]["median_ms"], 2)
    out["ratio_packed_diff_over_docs_diff_per_pair"] = round(per("packed_diff", k) / per("docs_diff", len(docs)), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks every shape (a rehearsal); 1.0 = the shapes above")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    eng = crdt_amd.Engine(int(os.environ.get("YCRDT_DEVICE", "0")))
    rng = random.Random(286)
    res = {"probe": "sync_docs", "version": crdt_amd.lib().ycrdt_version().decode(), "scale": a.scale, "shapes": {}}

    # (i), (ii): one C2-shaped document, merged on its own (marks)
    cfg = dict(workload.C2)
    cfg["n_replicas"] = max(4, int(cfg["n_replicas"] * a.scale))
    cfg["n_keys"] = max(100, int(cfg["n_keys"] * a.scale))
    ups, _ = workload.gen_map(**cfg)
    d = crdt_amd.Doc(client_id=0x7FFFFFF0, engine=eng)
    d.apply_updates(ups)
    d.flush()
    sv = read_sv(d.encode_state_vector())
    res["c2_state_bytes"] = len(d.encode_state_as_update())
    res["c2_clients"] = len(sv)
    npeers = max(4, int(256 * a.scale))
    svs = []
    for _ in range(npeers):
        e = list(sv)
        for j in rng.sample(range(len(e)), min(3, len(e))):
            e[j] = (e[j][0], max(0, e[j][1] - rng.randint(1, 5)))
        svs.append(write_sv(e))
    res["shapes"]["c2_lagging"] = measure(eng, [d] * npeers, svs, [d], res["c2_state_bytes"], 2, a.repeats)
    nj = max(2, int(16 * a.scale))
    res["shapes"]["c2_joiners"] = measure(eng, [d] * nj, [b""] * nj, [d], res["c2_state_bytes"], 2, a.repeats)

    # (iii): a fleet of small documents, merged together (no marks)
    with open(os.path.join(ROOT, "tests", "golden", "configs.json")) as f:
        cases = [c for c in json.load(f)["cases"] if c["name"].startswith("c5_") and c["diffs"]]
    nd = max(4, int(10_000 * a.scale))
    docs = [crdt_amd.Doc(client_id=0x7FFFFFF0, engine=eng) for _ in range(nd)]
    pairs = [(i, bytes.fromhex(u)) for i in range(nd) for u in cases[i % len(cases)]["updates"]]
    crdt_amd.apply_updates_multi([docs[i] for i, _ in pairs], [u for _, u in pairs], engine=eng)
    fsvs = [bytes.fromhex(cases[i % len(cases)]["diffs"][0]["sv"]) for i in range(nd)]
    res["shapes"]["c5_fleet"] = measure(eng, docs, fsvs, docs, max(len(c["state"]) // 2 for c in cases), 2, a.repeats)

    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
