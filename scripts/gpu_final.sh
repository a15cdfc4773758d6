#!/bin/bash
# Rehearsal on one GPU: every -m gpu test, smoke(), then the benchmark with every side leg (--full).
# Logs and the bench line go to $OUT (default run_out/).
set -u
OUT=${OUT:-run_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 900 python -u -m pytest tests -x -q --timeout 300 --timeout-method thread -m gpu > "$OUT/final_tests.log" 2>&1
rc=$?; echo "[tests] rc=$rc"; tail -n 3 "$OUT/final_tests.log"; [ $rc -eq 0 ] || { tail -40 "$OUT/final_tests.log"; exit $rc; }
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > "$OUT/final_smoke.log" 2>&1 || { tail -20 "$OUT/final_smoke.log"; exit 1; }
tail -1 "$OUT/final_smoke.log"
timeout -k 10 1000 python -u bench.py --full > "$OUT/final_bench.json" 2> "$OUT/final_bench.err" || { tail -20 "$OUT/final_bench.err"; exit 1; }
python3 scripts/bench_summary.py "$OUT/final_bench.json"
