#!/bin/bash
# Clean per-step rocprofv3 tables of the shipped headline step, the att8 step
# and the beam-5 decode, plus back-to-back device stamps of the headline step.
export OUT=${OUT:-bench_out}  # output directory (inherited by the scripts called from here)
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
TAG=${TAG:-prof}
mkdir -p $OUT
prof() {  # name, delimiter, steps, bench args...
  local name=$1 delim=$2 n=$3; shift 3
  rm -rf $OUT/prof_${TAG}_$name
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${TAG}_$name \
    -o $name -- python bench.py --full "$@" > $OUT/prof_${TAG}_$name.log 2>&1 || return $?
  python scripts/prof_steps.py $OUT/prof_${TAG}_$name/${name}_kernel_trace.csv $n 40 $delim \
    > $OUT/steps_${TAG}_$name.txt && head -n 16 $OUT/steps_${TAG}_$name.txt
  rm -f $OUT/prof_${TAG}_$name/${name}_kernel_trace.csv
}
prof head adam_update_kernel 10 --steps 10 --warmup 5 --att8 0 --beam5 0 --cst 0 || exit $?
prof att8 adam_update_kernel 10 --steps 10 --warmup 5 --num_chunks 8 --att8 0 --beam5 0 --cst 0 || exit $?
prof beam beam_fused_step_kernel 27 --mode beam --steps 4 --warmup 3 --att8 0 --beam5 0 --cst 0 || exit $?
timeout -k 10 300 python bench.py --full --stamps 4 --att8 0 --beam5 0 --cst 0 > $OUT/stamps_$TAG.json 2> $OUT/stamps_$TAG.err || exit $?
grep -A60 "stamps (us" $OUT/stamps_$TAG.err | head -60
