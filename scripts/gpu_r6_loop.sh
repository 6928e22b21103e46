#!/bin/bash
# round 6: persistent reverse loop -- numerics tests, then interleaved A/B
export OUT=${OUT:-bench_out}  # output directory (inherited by the scripts called from here)
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 300 python -u -m pytest -x -v --timeout 120 --timeout-method thread -p no:cacheprovider \
  tests/test_gpu_bwd_loop.py > $OUT/pytest_r6_loop.log 2>&1 || { tail -40 $OUT/pytest_r6_loop.log; exit 1; }
tail -3 $OUT/pytest_r6_loop.log
timeout -k 10 400 python -u -m pytest -x -q --timeout 120 --timeout-method thread -p no:cacheprovider \
  tests/test_gpu_headline.py tests/test_gpu_graph.py tests/test_gpu_kernels.py > $OUT/pytest_r6_loop2.log 2>&1 || { tail -40 $OUT/pytest_r6_loop2.log; exit 1; }
tail -2 $OUT/pytest_r6_loop2.log
ARMS="steps:CSTCAP_BWD_LOOP=0 loop:CSTCAP_BWD_LOOP=1" REPS=2 TAG=loop bash scripts/gpu_ab.sh || exit $?
timeout -k 10 300 python bench.py --stamps 4 --att8 0 --beam5 0 --cst 0 --xe 0 > $OUT/stamps_loop.json 2> $OUT/stamps_loop.err || exit $?
grep -A40 "stamps (us" $OUT/stamps_loop.err | head -40
