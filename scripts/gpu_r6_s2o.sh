#!/bin/bash
# round 6 session 2: hipBLASLt candidates timed per tuned shape, 32 (default) vs 128
export OUT=${OUT:-bench_out}  # output directory (inherited by the scripts called from here)
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
mkdir -p $OUT/s2o
for i in 1 2; do
  for m in 128 32; do
    CSTCAP_BLASLT_NCAND=$m timeout -k 10 300 python bench.py --full --att8 0 --beam5 0 --cst 0 > $OUT/s2o/n${m}_$i.log 2>&1 || { tail -20 $OUT/s2o/n${m}_$i.log; exit 1; }
    grep '^{' $OUT/s2o/n${m}_$i.log > $OUT/s2o/n${m}_$i.json
    python -c "
import json; d=json.load(open('$OUT/s2o/n${m}_$i.json'))
print('ncand=$m scst', d['ms_per_step'], 'xe', d['xe']['ms_per_step'], [(c['m'],c['n'],c['k'],c['candidate'],c['us']) for c in d['blaslt_x_choice']])"
  done
done
