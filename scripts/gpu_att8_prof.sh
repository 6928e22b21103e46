#!/bin/bash
# rocprofv3 per-step kernel table of the att8 step (bench --num_chunks 8) and
# the last step's reverse-loop launch sequence (step kernel / attention
# backward), for the fused attention backward (lstm.hip).
export OUT=${OUT:-bench_out}  # output directory (inherited by the scripts called from here)
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
TAG=${TAG:-att8}
mkdir -p $OUT
rm -rf $OUT/prof_$TAG
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o att8 -- \
  python bench.py --steps 6 --warmup 4 --num_chunks ${NUMCH:-8} --att8 0 --beam5 0 --cst 0 ${BENCH_ARGS} \
  > $OUT/prof_$TAG.log 2>&1 || exit $?
python scripts/prof_steps.py $OUT/prof_$TAG/att8_kernel_trace.csv 5 45 adam_update_kernel \
  "${SEQ-lstm_step_bwd|att_bwd|att_dgv}" > $OUT/steps_$TAG.txt && head -n 30 $OUT/steps_$TAG.txt
rm -f $OUT/prof_$TAG/att8_kernel_trace.csv
