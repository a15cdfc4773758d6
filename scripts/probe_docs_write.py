#!/usr/bin/env python3
"""Probe of the fleet writes (ycrdt_docs_write): one `users` key of every document set in two ways.

The fleet is the C5 shape of scripts/probe_docs_read.py: 20 000 documents of 2-3 small replica
updates each (50 seeded bases, cycled), ingested with one apply_updates_multi call. Two twin fleets
with equal client ids hold the same documents. Every document sets one key its `users` map holds.
  (a) docs_write  one crdt_amd.docs_write call over all documents of fleet A (one multi-document
                  merge, the view, one lane per op), with its device_ms;
  (b) map_set     the loop of Doc.map_set over fleet B: a merge, the view kernels, the view's copy to
                  the host and a host index per document before its small host encode.
Both run in one process and alternate. Before every repeat each document of both fleets ingests one
more small update (apply_updates_multi, not timed), as a message round does: that is what makes the
per-document views stale, so that (b) pays what it pays when it writes after an ingest. Each way is
warmed up once first. Times are host wall clock around calls that end in a synchronise; medians,
minimum and maximum over the repeats. In every repeat the updates of (a) must equal the
take_local_update of (b) byte for byte (taken outside the timed loop). Accepted when (a)'s median
lies below (b)'s by more than (b)'s own max - min spread.

  python scripts/probe_docs_write.py [--docs 20000] [--repeats 5] [--out FILE]
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
from scripts.probe_docs_json import round_update, spread, vu  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "docs_write_fleet.json"))
    a = ap.parse_args()

    base = [workload.gen_map(n_keys=20, n_replicas=2 + s % 2, ops_per_replica=4, seed=700 + s)[0] for s in range(50)]
    n = a.docs
    fleets = [[crdt_amd.Doc(client_id=0x10000000 + i) for i in range(n)] for _ in range(2)]
    idx, ups = [], []
    for i in range(n):
        for u in base[i % len(base)]:
            idx.append(i)
            ups.append(u)
    t0 = time.perf_counter()
    crdt_amd.apply_updates_multi(fleets[0], ups, doc_index=idx)
    ingest_ms = (time.perf_counter() - t0) * 1e3
    crdt_amd.apply_updates_multi(fleets[1], ups, doc_index=idx)
    A, B = fleets
    for d in B:
        d.track_local(True)
    # a recorded key of every base's `users` map (the last in entry order)
    base_key = [sorted(json.loads(A[b].root_json("users", "map")))[-1] for b in range(len(base))]
    keys = [base_key[i % len(base)] for i in range(n)]

    def value(r):
        text = f"written in round {r}".encode()
        return bytes([119]) + vu(len(text)) + text

    def way_a(r):
        v = value(r)
        ops = [("map_set", d, "users", (k, v)) for d, k in zip(A, keys)]
        t = time.perf_counter()
        got, codes, st = crdt_amd.docs_write_stats(ops)
        return (time.perf_counter() - t) * 1e3, got, codes, st

    def way_b(r):
        v = value(r)
        t = time.perf_counter()
        for d, k in zip(B, keys):
            d.map_set("users", k, v)
        ms = (time.perf_counter() - t) * 1e3
        return ms, [d.take_local_update() for d in B]

    def message_round(r):
        u = round_update(r)
        for fleet in fleets:
            crdt_amd.apply_updates_multi(fleet, [u] * n, doc_index=list(range(n)))

    message_round(0)
    way_a(0)  # warm-up of each way (on both fleets the same op: they stay twins)
    way_b(0)
    ta, tb, dev, equal, stats = [], [], [], True, None
    for r in range(a.repeats):
        message_round(1 + r)  # (both ways of this repeat write after it: only (b) keeps per-document views, stale now)
        ms_a, got_a, codes, stats = way_a(1 + r)
        ms_b, got_b = way_b(1 + r)
        ta.append(ms_a)
        tb.append(ms_b)
        dev.append(stats["device_ms"])
        equal = equal and got_a == got_b and not any(codes) and all(got_a)
        print(f"repeat {r}: docs_write {ms_a:.1f} ms (device {stats['device_ms']:.1f}), map_set loop {ms_b:.1f} ms, "
              f"equal {got_a == got_b}, {stats}", file=sys.stderr, flush=True)
    med_a, med_b = statistics.median(ta), statistics.median(tb)
    res = {
        "probe": "docs_write_fleet",
        "docs": n,
        "ops": n,
        "repeats": a.repeats,
        "ingest_ms": round(ingest_ms, 3),
        "out_bytes": stats["out_bytes"],
        "stats": stats,
        "docs_write": spread(ta),
        "docs_write_device_ms": spread(dev),
        "map_set_loop": spread(tb),
        "ratio_median_b_over_a": round(med_b / med_a, 2),
        "accepted": med_b - med_a > max(tb) - min(tb),
        "equal_bytes": equal,
    }
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
