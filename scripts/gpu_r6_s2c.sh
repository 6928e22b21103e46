#!/bin/bash
# round 6 session 2: split-bf16 FeatPool (LDS-staged) -- featpool + attention
# tests, att8 / headline bench, att8 step table
export OUT=${OUT:-bench_out}  # output directory (inherited by the scripts called from here)
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
mkdir -p $OUT/s2c
timeout -k 10 600 python -u -m pytest -x -v --timeout 300 --timeout-method thread -p no:cacheprovider \
  tests/test_gpu_kernels.py -k "featpool" tests/test_gpu_attention_headline.py tests/test_gpu_attention.py \
  > $OUT/s2c/pytest.log 2>&1 || { tail -40 $OUT/s2c/pytest.log; exit 1; }
tail -1 $OUT/s2c/pytest.log
for i in 1 2; do
  timeout -k 10 300 python bench.py --num_chunks 8 --att8 0 --beam5 0 --cst 0 --xe 0 > $OUT/s2c/att8_$i.log 2>&1 || { tail -20 $OUT/s2c/att8_$i.log; exit 1; }
  grep '^{' $OUT/s2c/att8_$i.log > $OUT/s2c/att8_$i.json
  python -c "import json; d=json.load(open('$OUT/s2c/att8_$i.json')); print('att8', d['ms_per_step'], 'err', d['device_errors'])"
  timeout -k 10 300 python bench.py --full --att8 0 --beam5 0 --cst 0 > $OUT/s2c/head_$i.log 2>&1 || { tail -20 $OUT/s2c/head_$i.log; exit 1; }
  grep '^{' $OUT/s2c/head_$i.log > $OUT/s2c/head_$i.json
  python -c "import json; d=json.load(open('$OUT/s2c/head_$i.json')); print('scst', d['ms_per_step'], 'xe', d['xe']['ms_per_step'], 'err', d['device_errors'])"
done
rm -rf $OUT/s2c/prof
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d $OUT/s2c/prof -o att8 -- \
    python bench.py --steps 6 --warmup 4 --num_chunks 8 --att8 0 --beam5 0 --cst 0 --xe 0 > $OUT/s2c/prof.log 2>&1 || exit $?
python scripts/prof_steps.py $OUT/s2c/prof/att8_kernel_trace.csv 5 40 adam_update_kernel 'e' > $OUT/s2c/steps_att8.txt || exit $?
rm -f $OUT/s2c/prof/att8_kernel_trace.csv
grep -i "featpool\|^window" $OUT/s2c/steps_att8.txt | head -8
