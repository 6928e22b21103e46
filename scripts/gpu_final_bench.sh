#!/bin/bash
# the driver's round-end commands on the final tree: GPU suite, smoke, bench
export OUT=${OUT:-bench_out}  # output directory (inherited by the scripts called from here)
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 700 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread -p no:cacheprovider > $OUT/pytest_gpu_final.log 2>&1 || exit $?
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/smoke_final.log 2>&1 || exit $?
timeout -k 10 300 python bench.py --full > $OUT/bench_final.log 2>&1 || exit $?
grep '^{' $OUT/bench_final.log
