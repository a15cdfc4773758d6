#!/usr/bin/env python3
"""Probe of the fleet point reads (ycrdt_docs_read): one `users` key of every document, read three ways.

The fleet is the C5 shape of scripts/probe_docs_json.py: 20 000 documents of 2-3 small replica
updates each (50 seeded bases, cycled), ingested with one apply_updates_multi call. Every document is
asked for one key its `users` map holds.
  (a) docs_read   one crdt_amd.docs_read call over all documents (one multi-document merge, the view,
                  one lane per read), with its device_ms;
  (b) map_get     the loop of Doc.map_get over the same documents: a merge, the view kernels, the
                  view's copy to the host and a host index per document;
  (c) docs_json   one crdt_amd.docs_json call for every `users` root and a host pick of the key
                  (json.loads of each text): reported, not gated.
All run in one process and alternate. Before every repeat each document ingests one more small update
(apply_updates_multi, not timed), as a message round does: that is what makes the per-document views
stale, so that (b) pays what it pays when it serves after an ingest and not a cached read. Each way
is warmed up once first. Times are host wall clock around calls that end in a synchronise; medians,
minimum and maximum over the repeats. (a) must equal (b) byte for byte in every repeat. Accepted when
(a)'s median lies below (b)'s by more than (b)'s own max - min spread.

  python scripts/probe_docs_read.py [--docs 20000] [--repeats 5] [--out FILE]
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
from scripts.probe_docs_json import round_update, spread  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "docs_read_fleet.json"))
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
    # a recorded key of every base's `users` map (the last in entry order)
    base_key = [sorted(json.loads(docs[b].root_json("users", "map")))[-1] for b in range(len(base))]
    keys = [base_key[i % len(base)] for i in range(n)]
    reads = [("map_get", d, "users", k) for d, k in zip(docs, keys)]
    roots = ["users"] * n

    def way_a():
        t = time.perf_counter()
        got, st = crdt_amd.docs_read_stats(reads)
        return (time.perf_counter() - t) * 1e3, got, st

    def way_b():
        t = time.perf_counter()
        got = [d.map_get("users", k) for d, k in zip(docs, keys)]
        return (time.perf_counter() - t) * 1e3, got

    def way_c():
        t = time.perf_counter()
        texts = crdt_amd.docs_json(docs, roots, "map")
        got = [json.loads(x)[k] for x, k in zip(texts, keys)]
        return (time.perf_counter() - t) * 1e3, got

    def message_round(r):
        u = round_update(r)
        crdt_amd.apply_updates_multi(docs, [u] * n, doc_index=list(range(n)))

    message_round(0)
    way_a()  # warm-up of each way
    message_round(1)
    way_b()
    message_round(2)
    way_c()
    ta, tb, tc, dev, equal, picked, stats = [], [], [], [], True, True, None
    for r in range(a.repeats):
        message_round(3 + r)  # (every way of this repeat reads after it: only (b) keeps per-document views, stale now)
        ms_a, got_a, stats = way_a()
        ms_c, got_c = way_c()
        ms_b, got_b = way_b()
        ta.append(ms_a)
        tb.append(ms_b)
        tc.append(ms_c)
        dev.append(stats["device_ms"])
        equal = equal and got_a == got_b
        picked = picked and all(s == 1 and json.loads(x) == v for (s, x), v in zip(got_a, got_c))
        print(f"repeat {r}: docs_read {ms_a:.1f} ms (device {stats['device_ms']:.1f}), map_get loop {ms_b:.1f} ms, "
              f"docs_json + pick {ms_c:.1f} ms", file=sys.stderr, flush=True)
    med_a, med_b = statistics.median(ta), statistics.median(tb)
    res = {
        "probe": "docs_read_fleet",
        "docs": n,
        "reads": n,
        "repeats": a.repeats,
        "ingest_ms": round(ingest_ms, 3),
        "out_bytes": stats["out_bytes"],
        "stats": stats,
        "docs_read": spread(ta),
        "docs_read_device_ms": spread(dev),
        "map_get_loop": spread(tb),
        "docs_json_and_pick": spread(tc),
        "ratio_median_b_over_a": round(med_b / med_a, 2),
        "ratio_median_c_over_a": round(statistics.median(tc) / med_a, 2),
        "accepted": med_b - med_a > max(tb) - min(tb),
        "equal_bytes": equal,
        "equal_to_docs_json_pick": picked,
    }
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0 if equal and picked else 1


if __name__ == "__main__":
    sys.exit(main())
