#!/bin/bash
# round 6: DP stand-in priority study (1-rank RCCL)
export OUT=${OUT:-bench_out}  # output directory (inherited by the scripts called from here)
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 400 python scripts/dp_standin.py 29517 32 400 10 > $OUT/dp_standin.json 2> $OUT/dp_standin.err || { tail -20 $OUT/dp_standin.err; exit 1; }
cat $OUT/dp_standin.json
