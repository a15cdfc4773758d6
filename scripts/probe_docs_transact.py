#!/usr/bin/env python3
"""Probe of the fleet transactions (ycrdt_docs_transact): every document runs a queue of ops that
depend on one another, in two ways.

The fleet is the C5 shape of scripts/probe_docs_write.py: 20 000 documents of 2-3 small replica
updates each (50 seeded bases, cycled), ingested with one apply_updates_multi call. Two twin fleets
with equal client ids hold the same documents.

Dependent workload, per document and repeat: a YArray set under a fresh key of `users`, one value
pushed into it (crdt.js:422-431), and two sets of one recorded key — four ops, three of them planned
through an earlier one.
  (a) docs_transact  one crdt_amd.docs_transact call over fleet A;
  (b) docs_write     one crdt_amd.docs_write call with the same ops over fleet B: every document's ops
                     depend on one another, so all of them go through the single calls in order — what
                     a caller had before ycrdt_docs_transact.
Independent workload (a guard): probe_docs_write.py's one map_set per document through both calls;
both stay on the device, docs_transact through its own planning kernel.

Both ways run in one process and alternate. Before every repeat each document of both fleets ingests
one more small update (apply_updates_multi, not timed), as a message round does. Each way is warmed up
once first. Times are host wall clock around calls that end in a synchronise; medians, minimum and
maximum over the repeats. In every repeat the updates and codes of the two ways must be equal byte for
byte. Accepted when (a)'s median lies below (b)'s by more than (b)'s own max - min spread, and when on
the independent workload docs_transact is not slower than docs_write by more than the larger of the
two spreads.

  python scripts/probe_docs_transact.py [--docs 20000] [--repeats 5] [--out FILE]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "docs_transact_fleet.json"))
    a = ap.parse_args()

    base = [workload.gen_map(n_keys=20, n_replicas=2 + s % 2, ops_per_replica=4, seed=700 + s)[0] for s in range(50)]
    n = a.docs
    fleets = [[crdt_amd.Doc(client_id=0x10000000 + i) for i in range(n)] for _ in range(2)]
    idx, ups = [], []
    for i in range(n):
        for u in base[i % len(base)]:
            idx.append(i)
            ups.append(u)
    for fleet in fleets:
        crdt_amd.apply_updates_multi(fleet, ups, doc_index=idx)
    A, B = fleets
    base_key = [sorted(json.loads(A[b].root_json("users", "map")))[-1] for b in range(len(base))]
    keys = [base_key[i % len(base)] for i in range(n)]

    def value(text):
        text = text.encode()
        return bytes([119]) + vu(len(text)) + text

    def dependent(fleet, r):
        v1, v2, fresh = value(f"first in round {r}"), value(f"second in round {r}"), f"list {r}"
        ops = []
        for d, k in zip(fleet, keys):
            ops += [("map_set_type", d, "users", (fresh, 0)), ("array_push", d, "users", [v1], fresh), ("map_set", d, "users", (k, v1)),
                    ("map_set", d, "users", (k, v2))]
        return ops

    def independent(fleet, r):
        v = value(f"written in round {r}")
        return [("map_set", d, "users", (k, v)) for d, k in zip(fleet, keys)]

    def timed(call, ops):
        t = time.perf_counter()
        got, codes, st = call(ops)
        return (time.perf_counter() - t) * 1e3, got, codes, st

    def message_round(r):
        u = round_update(r)
        for fleet in fleets:
            crdt_amd.apply_updates_multi(fleet, [u] * n, doc_index=list(range(n)))

    def run(label, make, first_round):
        """(a) docs_transact over A and (b) docs_write over B, alternating; the fleets stay twins."""
        message_round(first_round)
        timed(crdt_amd.docs_transact_stats, make(A, first_round))  # warm-up of each way
        timed(crdt_amd.docs_write_stats, make(B, first_round))
        ta, tb, dev_a, dev_b, equal, st_a, st_b = [], [], [], [], True, None, None
        for r in range(first_round + 1, first_round + 1 + a.repeats):
            message_round(r)
            ms_a, got_a, codes_a, st_a = timed(crdt_amd.docs_transact_stats, make(A, r))
            ms_b, got_b, codes_b, st_b = timed(crdt_amd.docs_write_stats, make(B, r))
            ta.append(ms_a)
            tb.append(ms_b)
            dev_a.append(st_a["device_ms"])
            dev_b.append(st_b["device_ms"])
            same = got_a == got_b and codes_a == codes_b and not any(codes_a) and all(got_a)
            equal = equal and same
            print(f"{label} repeat {r}: docs_transact {ms_a:.1f} ms (device {st_a['device_ms']:.1f}), docs_write {ms_b:.1f} ms, equal {same}, "
                  f"{st_a} / {st_b}", file=sys.stderr, flush=True)
        return {
            "ops": len(make(A, 0)),
            "docs_transact": spread(ta),
            "docs_transact_device_ms": spread(dev_a),
            "docs_transact_stats": st_a,
            "docs_write": spread(tb),
            "docs_write_device_ms": spread(dev_b),
            "docs_write_stats": st_b,
            "ratio_median_write_over_transact": round(statistics.median(tb) / statistics.median(ta), 2),
            "equal_bytes": equal,
        }, ta, tb

    dep, ta, tb = run("dependent", dependent, 0)
    dep["accepted"] = statistics.median(tb) - statistics.median(ta) > max(tb) - min(tb)
    ind, ta, tb = run("independent", independent, 100)
    ind["accepted"] = statistics.median(ta) - statistics.median(tb) <= max(max(ta) - min(ta), max(tb) - min(tb))
    res = {"probe": "docs_transact_fleet", "docs": n, "repeats": a.repeats, "dependent": dep, "independent": ind,
           "accepted": dep["accepted"] and ind["accepted"], "equal_bytes": dep["equal_bytes"] and ind["equal_bytes"]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0 if res["equal_bytes"] else 1


if __name__ == "__main__":
    sys.exit(main())
