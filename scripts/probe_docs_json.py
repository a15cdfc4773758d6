#!/usr/bin/env python3
"""Probe of the fleet toJSON path (ycrdt_docs_json): every document's `users` root, read two ways.

The fleet is the C5 shape of tests/test_gpu_multidoc.py::test_apply_multi_c5_fleet_large: 20 000
documents of 2-3 small replica updates each (50 seeded bases, cycled), ingested with one
apply_updates_multi call.
  (a) docs_json   one crdt_amd.docs_json call over all documents (one multi-document merge, the view,
                  the JSON text written on the device), with its device_ms;
  (b) root_json   the loop of Doc.root_json over the same documents: a merge, the view kernels, two
                  or three synchronisations and a host-side JSON writer per document.
Both run in one process and alternate. Before every repeat each document ingests one more small
update (apply_updates_multi, not timed), as a message round does: that is what invalidates the
per-document views, so that (b) pays what it pays after an ingest and not a cached read. Each way
is warmed up once first. Times are host wall clock around calls that end in a synchronise; medians,
minimum and maximum over the repeats. (a) must equal (b) byte for byte in every repeat.

A last line reads one C2-shaped document's `users` root both ways (not a goal of the batch path).

  python scripts/probe_docs_json.py [--docs 20000] [--repeats 5] [--no-c2] [--out FILE]
"""
import argparse
import json
import os
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


def round_update(r):
    """One YMap set on root 'users' by a client of its own: [1 section][1 struct][client][clock 0]
    info 0x28 (Any, parentSub), parent root 'users', key 'round<r>', one value."""
    key = f"round{r}".encode()
    return vu(1) + vu(1) + vu(0x40000000 + r) + vu(0) + bytes([0x28, 1, 5]) + b"users" + vu(len(key)) + key + bytes([1, 125, r % 64, 0])


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "all_ms": [round(x, 3) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-c2", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "docs_json_fleet.json"))
    a = ap.parse_args()

    base = [workload.gen_map(n_keys=20, n_replicas=2 + s % 2, ops_per_replica=4, seed=700 + s)[0] for s in range(50)]
    n = a.docs
    docs = [crdt_amd.Doc(client_id=0x7FFFFFF0) for _ in range(n)]
    idx, ups = [], []
    for i in range(n):
        for u in base[i % len(base)]:
            idx.append(i)
            ups.append(u)
    t0 = time.perf_counter()
    crdt_amd.apply_updates_multi(docs, ups, doc_index=idx)
    ingest_ms = (time.perf_counter() - t0) * 1e3
    roots = ["users"] * n

    def way_a():
        t = time.perf_counter()
        texts, st = crdt_amd.docs_json_stats(docs, roots, "map")
        return (time.perf_counter() - t) * 1e3, texts, st

    def way_b():
        t = time.perf_counter()
        texts = [d.root_json("users", "map") for d in docs]
        return (time.perf_counter() - t) * 1e3, texts

    def message_round(r):
        u = round_update(r)
        crdt_amd.apply_updates_multi(docs, [u] * n, doc_index=list(range(n)))

    message_round(0)
    way_a()  # warm-up of each way
    message_round(1)
    way_b()
    ta, tb, dev, equal, stats = [], [], [], True, None
    for r in range(a.repeats):
        message_round(2 + r)
        ms_a, texts_a, stats = way_a()
        ms_b, texts_b = way_b()
        ta.append(ms_a)
        tb.append(ms_b)
        dev.append(stats["device_ms"])
        equal = equal and texts_a == texts_b
        print(f"repeat {r}: docs_json {ms_a:.1f} ms (device {stats['device_ms']:.1f}), root_json loop {ms_b:.1f} ms", file=sys.stderr, flush=True)
    res = {
        "probe": "docs_json_fleet",
        "docs": n,
        "requests": n,
        "repeats": a.repeats,
        "ingest_ms": round(ingest_ms, 3),
        "out_bytes": stats["out_bytes"],
        "stats": stats,
        "docs_json": spread(ta),
        "docs_json_device_ms": spread(dev),
        "root_json_loop": spread(tb),
        "ratio_median": round(statistics.median(tb) / statistics.median(ta), 2),
        "equal_bytes": equal,
    }
    if not a.no_c2:
        cfg = dict(workload.C2)
        d = crdt_amd.Doc(client_id=0x7FFFFFF0)
        d.apply_updates(workload.gen_map(**cfg)[0])
        d.flush()
        one_a, one_b = [], []
        same = True
        for r in range(3):
            d.apply_update(round_update(100 + r))
            d.flush()
            t = time.perf_counter()
            texts, st1 = crdt_amd.docs_json_stats([d], ["users"], "map")
            one_a.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            single = d.root_json("users", "map")
            one_b.append((time.perf_counter() - t) * 1e3)
            same = same and texts[0] == single
        res["c2_one_document"] = {"docs_json": spread(one_a), "root_json": spread(one_b), "json_bytes": len(single),
                                  "pairs_device": st1["pairs_device"], "equal_bytes": same}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
