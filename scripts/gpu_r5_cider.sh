#!/bin/bash
# CIDEr-D kernel timing at the bench shapes (scripts/microbench_cider.py)
export OUT=${OUT:-bench_out}  # output directory (inherited by the scripts called from here)
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 300 python scripts/microbench_cider.py > $OUT/cider_${TAG:-r5}.json 2> $OUT/cider_${TAG:-r5}.err || exit $?
cat $OUT/cider_${TAG:-r5}.json
