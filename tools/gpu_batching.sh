#!/bin/bash
# Launch-batching A/B: runner tests, then the same short bench window with and without holding
# launches for min_launch_rows.
set -o pipefail
OUT=${OUT:-bench_logs}   # where the logs go (relative to the repository root)
mkdir -p $OUT/lb
timeout -k 10 300 python -u -m pytest tests/test_selfplay_gpu.py -m gpu -x -v --timeout 200 --timeout-method thread \
    > $OUT/lb/tests.log 2>&1 || { echo "selfplay tests failed"; tail -30 $OUT/lb/tests.log; exit 1; }
timeout -k 10 300 python bench.py --full --steps 3000 --no-cpu-baseline --min-launch-rows 0 > $OUT/lb/a.log 2>&1 || { echo "A failed"; tail $OUT/lb/a.log; exit 1; }
tail -1 $OUT/lb/a.log
timeout -k 10 300 python bench.py --full --steps 3000 --no-cpu-baseline > $OUT/lb/b.log 2>&1 || { echo "B failed"; tail $OUT/lb/b.log; exit 1; }
tail -1 $OUT/lb/b.log
timeout -k 10 300 python bench.py --full --steps 3000 --no-cpu-baseline --min-launch-rows 1024 --max-launch-wait-us 3000 > $OUT/lb/c.log 2>&1 || { echo "C failed"; tail $OUT/lb/c.log; exit 1; }
tail -1 $OUT/lb/c.log
echo ALL OK
