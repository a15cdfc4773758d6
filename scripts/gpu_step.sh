#!/bin/bash
# one GPU step: the rehearsal (every -m gpu test, smoke, bench.py --full), outputs under $OUT
set -u
export OUT=${OUT:-run_out}
export TMPDIR=/tmp
bash scripts/gpu_final.sh || exit 1
