#!/bin/bash
# rocprofv3 kernel trace of the headline bench + per-kernel summary and one
# step's timeline; extra bench args via BENCH_ARGS, output tag via TAG
export OUT=${OUT:-bench_out}  # output directory (inherited by the scripts called from here)
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
TAG=${TAG:-rc}
mkdir -p $OUT
rm -rf $OUT/prof_$TAG
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o $TAG -- python bench.py --full --steps 5 --warmup 3 --att8 0 $BENCH_ARGS > $OUT/prof_$TAG.log 2>&1 || exit $?
python scripts/prof_summary.py $OUT/prof_$TAG/${TAG}_kernel_trace.csv 5 45 > $OUT/prof_${TAG}_summary.txt
python scripts/step_timeline.py $OUT/prof_$TAG/${TAG}_kernel_trace.csv 1 > $OUT/step_timeline_$TAG.txt
