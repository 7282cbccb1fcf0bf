#!/bin/bash
# every -m gpu test, smoke(), and the default bench line with its CPU baseline (--full) (the driver's round-end sequence)
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 1000 python -u -m pytest tests -m gpu -x -q --timeout 500 --timeout-method thread > $OUT/final_tests.log 2>&1 || exit $?
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/final_smoke.log 2>&1 || exit $?
timeout -k 10 300 python bench.py --full > $OUT/final_bench.log 2>&1
