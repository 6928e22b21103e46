#!/bin/bash
# PMC counters of the eager step: headline config, then the 8-frame attention
# config, each in its own directory
export OUT=${OUT:-bench_out}  # output directory (inherited by the scripts called from here)
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
BENCH_ARGS="--att8 0" bash scripts/gpu_pmc.sh || exit $?
rm -rf $OUT/pmc_headline && mv $OUT/pmc $OUT/pmc_headline || exit $?
BENCH_ARGS="--num_chunks 8" bash scripts/gpu_pmc.sh || exit $?
rm -rf $OUT/pmc_att8 && mv $OUT/pmc $OUT/pmc_att8 || exit $?
