#!/bin/bash
# round 6 session 2: greedy MFMA attention (one row per video) + split-bf16 FeatPool
export OUT=${OUT:-bench_out}  # output directory (inherited by the scripts called from here)
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
mkdir -p $OUT/s2a
timeout -k 10 600 python -u -m pytest -x -v --timeout 300 --timeout-method thread -p no:cacheprovider \
  tests/test_gpu_attention_headline.py tests/test_gpu_attention.py tests/test_gpu_kernels.py \
  > $OUT/s2a/pytest.log 2>&1 || { tail -40 $OUT/s2a/pytest.log; exit 1; }
tail -1 $OUT/s2a/pytest.log
timeout -k 10 400 python bench.py --full --beam5 0 > $OUT/s2a/bench.log 2>&1 || { tail -20 $OUT/s2a/bench.log; exit 1; }
grep '^{' $OUT/s2a/bench.log > $OUT/s2a/bench.json
python -c "import json; d=json.load(open('$OUT/s2a/bench.json')); print('scst', d['ms_per_step'], 'cst', d['cst']['ms_per_step'], 'xe', d['xe']['ms_per_step'], 'att8', d['att8']['ms_per_step'], 'err', d['device_errors'])"
timeout -k 10 600 python -u -m pytest -x -q --timeout 300 --timeout-method thread -p no:cacheprovider \
  tests/test_gpu_headline.py tests/test_gpu_graph.py tests/test_gpu_cst.py \
  > $OUT/s2a/pytest2.log 2>&1 || { tail -40 $OUT/s2a/pytest2.log; exit 1; }
tail -1 $OUT/s2a/pytest2.log
