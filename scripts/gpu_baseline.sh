#!/bin/bash
# First GPU run: reference-semantics baseline (PyTorch ops, fp32, CPU CIDEr-D)
export OUT=${OUT:-bench_out}  # output directory (inherited by the scripts called from here)
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
export CSTCAP_ALLOW_TORCH_FALLBACK=1
mkdir -p $OUT
rocm-smi --showproductname > $OUT/smi.txt 2>&1 || true
timeout -k 10 600 python bench.py --full --impl torch --reward cpu --precision fp32 --dedupe_greedy 0 \
   --steps 5 --warmup 2 --json_out $OUT/ref_baseline.json > $OUT/ref_baseline.log 2>&1 && \
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_ref -o ref -- \
   python bench.py --full --impl torch --reward cpu --precision fp32 --dedupe_greedy 0 --steps 2 --warmup 1 \
   > $OUT/prof_ref.log 2>&1
echo "exit $?"
