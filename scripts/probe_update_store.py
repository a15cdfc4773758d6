#!/usr/bin/env python3
"""Probe of the doc-less update store: a persistence worker's two jobs over a fleet, each done two ways.

The fleet is the C5 shape of tests/test_gpu_multidoc.py::test_apply_multi_c5_fleet_large: 20 000
topics, each a log of 3-4 small updates (the states of 2-3 replicas and their deltas; 50 seeded
bases, cycled).

Compacting the logs (Y.mergeUpdates per topic):
  (a) merge_update_groups   one crdt_amd.merge_update_groups call over all topics, with its device_ms;
  (b) merge_updates loop    crdt_amd.merge_updates per topic: the code as it was before the batched
                            call, one device merge (launches and host synchronisations) per topic.
Refreshing the stored state vectors (Y.encodeStateVectorFromUpdate per stored update, the first of
every topic's log):
  (a) state_vectors_from_updates   one call over all of them;
  (b) temporary docs               what storeUpdate (crdt.js:28-77) does today: a fresh Doc,
                                   apply_update, encode_state_vector, per update.
  (b)'s bytes are compared with (a)'s only where the two mean the same thing: the update leaves
  nothing pending and starts every client at clock 0 (checked here for updates of one client
  section; a doc's state vector also counts what encodeStateVectorFromUpdate stops at).

Both ways of a job run in one process and alternate; each is warmed up once first. Times are host wall
clock around calls that end in a synchronise; median, minimum and maximum over the repeats. For the
merges (a) must equal (b) byte for byte in every repeat.

  python scripts/probe_update_store.py [--groups 20000] [--repeats 5] [--out FILE]
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


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "all_ms": [round(x, 3) for x in ms]}


def one_section_from_clock_0(u):
    """True for an update of exactly one client section that starts at clock 0 (the first section's
    header is the only one that can be read without parsing structs; the rest are not compared)."""
    p = 0
    vals = []
    for _ in range(4):  # sections, structs, client, clock
        v = s = 0
        while True:
            b = u[p]
            p += 1
            v |= (b & 0x7F) << s
            s += 7
            if b < 0x80:
                break
        vals.append(v)
        if vals[0] != 1:
            return False
    return vals[3] == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_store_fleet.json"))
    a = ap.parse_args()

    base = [workload.gen_map(n_keys=20, n_replicas=2 + s % 2, ops_per_replica=4, seed=700 + s)[0] for s in range(50)]
    n = a.groups
    groups = [list(base[i % len(base)]) for i in range(n)]
    firsts = [g[0] for g in groups]
    nupd = sum(len(g) for g in groups)

    def merge_a():
        t = time.perf_counter()
        got, st = crdt_amd.merge_update_groups_stats(groups)
        return (time.perf_counter() - t) * 1e3, got, st

    def merge_b():
        t = time.perf_counter()
        got = [crdt_amd.merge_updates(g) for g in groups]
        return (time.perf_counter() - t) * 1e3, got

    def sv_a():
        t = time.perf_counter()
        got, st = crdt_amd.state_vectors_from_updates_stats(firsts)
        return (time.perf_counter() - t) * 1e3, got, st

    def sv_b():
        t = time.perf_counter()
        got, pend = [], []
        for u in firsts:
            d = crdt_amd.Doc(client_id=0x7FFFFFF0)
            d.apply_update(u)
            got.append(d.encode_state_vector())
            pend.append(any(d.pending()))
        return (time.perf_counter() - t) * 1e3, got, pend

    for name, way in (("merge_update_groups", merge_a), ("merge_updates loop", merge_b), ("state_vectors_from_updates", sv_a),
                      ("temporary docs", sv_b)):  # warm-up of each way
        print(f"warm-up: {name} {way()[0]:.1f} ms", file=sys.stderr, flush=True)
    ma, mb, mdev, sa, sb, sdev = [], [], [], [], [], []
    merge_equal, sv_equal, sv_compared, mst, sst = True, True, 0, None, None
    for r in range(a.repeats):
        ms_a, got_a, mst = merge_a()
        ms_b, got_b = merge_b()
        ma.append(ms_a)
        mb.append(ms_b)
        mdev.append(mst["device_ms"])
        merge_equal = merge_equal and got_a == got_b
        print(f"repeat {r}: merge_update_groups {ms_a:.1f} ms (device {mst['device_ms']:.1f}), merge_updates loop {ms_b:.1f} ms",
              file=sys.stderr, flush=True)
        ts_a, svs_a, sst = sv_a()
        ts_b, svs_b, pend = sv_b()
        sa.append(ts_a)
        sb.append(ts_b)
        sdev.append(sst["device_ms"])
        sv_compared = 0
        for u, x, y, p in zip(firsts, svs_a, svs_b, pend):
            if p or not one_section_from_clock_0(u):
                continue
            sv_compared += 1
            sv_equal = sv_equal and x == y
        print(f"repeat {r}: state_vectors_from_updates {ts_a:.1f} ms (device {sst['device_ms']:.1f}), temporary docs {ts_b:.1f} ms",
              file=sys.stderr, flush=True)
    res = {
        "probe": "update_store_fleet",
        "groups": n,
        "updates": nupd,
        "repeats": a.repeats,
        "merge": {
            "stats": mst,
            "merge_update_groups": spread(ma),
            "merge_update_groups_device_ms": spread(mdev),
            "merge_updates_loop": spread(mb),
            "ratio_median": round(statistics.median(mb) / statistics.median(ma), 2),
            "below_by_more_than_the_loops_spread": statistics.median(mb) - statistics.median(ma) > max(mb) - min(mb),
            "equal_bytes": merge_equal,
        },
        "state_vectors": {
            "updates": len(firsts),
            "stats": sst,
            "state_vectors_from_updates": spread(sa),
            "state_vectors_from_updates_device_ms": spread(sdev),
            "temporary_docs": spread(sb),
            "ratio_median": round(statistics.median(sb) / statistics.median(sa), 2),
            "below_by_more_than_the_loops_spread": statistics.median(sb) - statistics.median(sa) > max(sb) - min(sb),
            "compared": sv_compared,
            "equal_bytes_where_compared": sv_equal,
        },
    }
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0 if merge_equal and sv_equal else 1


if __name__ == "__main__":
    sys.exit(main())
