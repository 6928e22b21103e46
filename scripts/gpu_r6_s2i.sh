#!/bin/bash
# round 6 session 2: host enqueue time per replayed step vs the synced step
export OUT=${OUT:-bench_out}  # output directory (inherited by the scripts called from here)
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
mkdir -p $OUT/s2i
timeout -k 10 300 python bench.py --sync_debug 1 --att8 0 --beam5 0 --cst 0 --xe 0 > $OUT/s2i/sd_scst.log 2>&1 || { tail -20 $OUT/s2i/sd_scst.log; exit 1; }
grep "sync_debug\|^{" $OUT/s2i/sd_scst.log | cut -c1-200
timeout -k 10 300 python bench.py --mode xe --sync_debug 1 --att8 0 --beam5 0 --cst 0 > $OUT/s2i/sd_xe.log 2>&1 || { tail -20 $OUT/s2i/sd_xe.log; exit 1; }
grep "sync_debug" $OUT/s2i/sd_xe.log
timeout -k 10 300 python bench.py --stamps 1 --att8 0 --beam5 0 --cst 0 --xe 0 > $OUT/s2i/stamps.log 2>&1 || { tail -20 $OUT/s2i/stamps.log; exit 1; }
grep '^{' $OUT/s2i/stamps.log > $OUT/s2i/stamps.json
python -c "import json; d=json.load(open('$OUT/s2i/stamps.json')); print(d.get('stamps_us'))"
