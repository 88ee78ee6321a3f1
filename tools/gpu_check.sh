#!/bin/bash
# GPU validation pass used during development: gpu tests, smoke, short bench.
set -o pipefail
OUT=${OUT:-bench_logs}   # where the logs go (relative to the repository root)
mkdir -p $OUT
timeout -k 10 400 python -m pytest tests -m gpu -x -q -s > $OUT/gpu_tests.log 2>&1 || { echo "gpu tests failed"; exit 1; }
timeout -k 10 150 python __graft_entry__.py > $OUT/smoke.log 2>&1 || { echo "smoke failed"; exit 1; }
timeout -k 10 420 python bench.py --full "$@" > $OUT/bench1.log 2>&1 || { echo "bench failed"; exit 1; }
echo ALL OK
