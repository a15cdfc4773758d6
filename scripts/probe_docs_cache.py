#!/usr/bin/env python3
"""Probe of the fleet cache refresh (ycrdt_docs_cache): every document's cache object `c`, three ways.

The fleet is the C5 shape of scripts/probe_docs_json.py: 20 000 documents of 2-3 small replica
updates each (50 seeded bases, cycled), ingested with one apply_updates_multi call. Every document
then gets, through one docs_write call, an index map `ix` that lists its `users` root as a map and a
small array root `log`, and three members of that array.
  (a) docs_cache  one crdt_amd.docs_cache call: one multi-document merge, the index read on the
                  device, the text of every `c` written on the device;
  (b) two calls   what the library offered before: docs_json of every `ix` root, json.loads of the
                  20 000 texts on the host, the (document, name, kind) triples from them, docs_json
                  of the listed roots. Timed up to the return of the second call; composing the
                  texts of `c` from its answers (needed here to compare bytes) is not timed;
  (c) loop        per document: Doc.root_json of `ix`, json.loads, Doc.root_json of every listed root.
All run in one process and alternate. Before every repeat each document ingests one more small
update (apply_updates_multi, not timed), as a message round does: that is what invalidates the
per-document views. Each way is warmed up once first. Times are host wall clock around calls that
end in a synchronise; medians, minimum and maximum over the repeats. (a) must equal the
composition of (b), and of (c), byte for byte in every repeat.

  python scripts/probe_docs_cache.py [--docs 20000] [--repeats 5] [--out FILE]
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


def any_str(s):
    return bytes([119]) + vu(len(s)) + s.encode()


def round_update(r):
    """One YMap set on root 'users' by a client of its own: [1 section][1 struct][client][clock 0]
    info 0x28 (Any, parentSub), parent root 'users', key 'round<r>', one value."""
    key = f"round{r}".encode()
    return vu(1) + vu(1) + vu(0x40000000 + r) + vu(0) + bytes([0x28, 1, 5]) + b"users" + vu(len(key)) + key + bytes([1, 125, r % 64, 0])


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "all_ms": [round(x, 3) for x in ms]}


def loosely_map(v):  # JavaScript's v == 'map' for a value that went through JSON
    while isinstance(v, list) and len(v) == 1:
        v = v[0]
    return v == "map"


def compose(names, texts):
    order = sorted(range(len(names)), key=lambda k: names[k].encode())
    return "{" + ",".join(json.dumps(names[k], ensure_ascii=False) + ":" + texts[k] for k in order) + "}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "docs_cache_fleet.json"))
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
    ops = []
    for i, d in enumerate(docs):
        ops.append(("map_set", d, "ix", ("users", any_str("map"))))
        ops.append(("map_set", d, "ix", ("log", any_str("array"))))
        ops.append(("array_push", d, "log", [bytes([125, i % 64]), any_str("entry"), bytes([120])]))
    _, codes, _ = crdt_amd.docs_write_stats(ops)
    assert not any(codes)

    def way_a():
        t = time.perf_counter()
        texts, st = crdt_amd.docs_cache_stats(docs)
        return (time.perf_counter() - t) * 1e3, texts, st

    def way_b():
        t = time.perf_counter()
        ix_texts, st1 = crdt_amd.docs_json_stats(docs, ["ix"] * n, "map")
        rd, rn, rk, first = [], [], [], []
        for d, t_ix in zip(docs, ix_texts):
            first.append(len(rd))
            for name, val in json.loads(t_ix).items():
                rd.append(d)
                rn.append(name)
                rk.append("map" if loosely_map(val) else "array")
        first.append(len(rd))
        texts, st2 = crdt_amd.docs_json_stats(rd, rn, rk)
        ms = (time.perf_counter() - t) * 1e3
        return ms, [compose(rn[first[i]:first[i + 1]], texts[first[i]:first[i + 1]]) for i in range(n)], st1["device_ms"], st2["device_ms"]

    def way_c():
        t = time.perf_counter()
        out = []
        for d in docs:
            ix = json.loads(d.root_json("ix", "map"))
            names = list(ix)
            out.append((names, [d.root_json(k, "map" if loosely_map(ix[k]) else "array") for k in names]))
        ms = (time.perf_counter() - t) * 1e3
        return ms, [compose(names, texts) for names, texts in out]

    def message_round(r):
        u = round_update(r)
        crdt_amd.apply_updates_multi(docs, [u] * n, doc_index=list(range(n)))

    message_round(0)
    way_a()  # warm-up of each way
    message_round(1)
    way_b()
    message_round(2)
    way_c()
    ta, tb, tc, dev_a, dev_b1, dev_b2, equal, stats = [], [], [], [], [], [], True, None
    for r in range(a.repeats):
        message_round(3 + r)
        ms_a, texts_a, stats = way_a()
        ms_b, texts_b, d1, d2 = way_b()
        ms_c, texts_c = way_c()
        ta.append(ms_a)
        tb.append(ms_b)
        tc.append(ms_c)
        dev_a.append(stats["device_ms"])
        dev_b1.append(d1)
        dev_b2.append(d2)
        equal = equal and texts_a == texts_b and texts_a == texts_c
        print(f"repeat {r}: docs_cache {ms_a:.1f} ms (device {stats['device_ms']:.1f}), two docs_json calls {ms_b:.1f} ms "
              f"(device {d1:.1f} + {d2:.1f}), root_json loop {ms_c:.1f} ms, equal {equal}", file=sys.stderr, flush=True)
    med_a, med_b = statistics.median(ta), statistics.median(tb)
    res = {
        "probe": "docs_cache_fleet",
        "docs": n,
        "repeats": a.repeats,
        "ingest_ms": round(ingest_ms, 3),
        "out_bytes": stats["out_bytes"],
        "stats": stats,
        "docs_cache": spread(ta),
        "docs_cache_device_ms": spread(dev_a),
        "two_docs_json_calls": spread(tb),
        "two_docs_json_calls_device_ms": {"ix": spread(dev_b1), "roots": spread(dev_b2)},
        "root_json_loop": spread(tc),
        "ratio_median_b_over_a": round(med_b / med_a, 2),
        "ratio_median_c_over_a": round(statistics.median(tc) / med_a, 2),
        "criterion_met": med_b - med_a > max(tb) - min(tb),
        "equal_bytes": equal,
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
