#!/bin/bash
# round 6: per-step rocprofv3 tables with fp16 pre on / off
export OUT=${OUT:-bench_out}  # output directory (inherited by the scripts called from here)
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
mkdir -p $OUT
for v in 0 1; do
  rm -rf $OUT/prof_p$v
  CSTCAP_PRE16=$v timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_p$v -o head -- python bench.py --steps 10 --warmup 5 --att8 0 --beam5 0 --cst 0 --xe 0 > $OUT/prof_p$v.log 2>&1 || exit $?
  python scripts/prof_steps.py $OUT/prof_p$v/head_kernel_trace.csv 10 14 adam_update_kernel > $OUT/steps_p$v.txt && head -n 16 $OUT/steps_p$v.txt
  rm -f $OUT/prof_p$v/head_kernel_trace.csv
done
