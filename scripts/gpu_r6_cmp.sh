#!/bin/bash
# round 6: XE vs SCST step on one box -- landmark launches of each step
export OUT=${OUT:-bench_out}  # output directory (inherited by the scripts called from here)
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 300 python -u -m pytest -x -q --timeout 200 --timeout-method thread -p no:cacheprovider \
  tests/test_gpu_graph.py tests/test_gpu_headline.py > $OUT/pytest_r6_cmp.log 2>&1 || { tail -30 $OUT/pytest_r6_cmp.log; exit 1; }
tail -1 $OUT/pytest_r6_cmp.log
for m in scst xe; do
  rm -rf $OUT/prof_$m
  timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d $OUT/prof_$m -o $m -- python bench.py --mode $m --steps 10 --warmup 5 --att8 0 --beam5 0 --cst 0 --xe 0 > $OUT/prof_$m.log 2>&1 || exit $?
  python scripts/prof_steps.py $OUT/prof_$m/${m}_kernel_trace.csv 10 30 adam_update_kernel 'e' > $OUT/steps_$m.txt || exit $?
  rm -f $OUT/prof_$m/${m}_kernel_trace.csv
  head -1 $OUT/steps_$m.txt
  sed -n 27,500p $OUT/steps_$m.txt | grep -E "Cijk|lstm_bwd_loop|adam_update|token_group_sum|_loss_fwd|vocab_exp_convert|cider_d|lstm_step_fwd" | cut -c1-100
done
