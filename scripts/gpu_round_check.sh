#!/bin/bash
# round-end style check: GPU tests, smoke(), headline + attention benches,
# rocprofv3 kernel trace + --stats of the headline (per-kernel summary, step timeline)
export OUT=${OUT:-bench_out}  # output directory (inherited by the scripts called from here)
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread -p no:cacheprovider > $OUT/pytest_gpu.log 2>&1 || exit $?
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/smoke.log 2>&1 || exit $?
timeout -k 10 300 python bench.py --full --steps 40 --warmup 5 --json_out $OUT/bench_hip.json > $OUT/bench_hip.log 2>&1 || exit $?
timeout -k 10 300 python bench.py --steps 30 --warmup 5 --num_chunks 8 --json_out $OUT/bench_att8.json > $OUT/bench_att8.log 2>&1 || exit $?
rm -rf $OUT/prof_rc
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_rc -o rc -- python bench.py --full --steps 5 --warmup 2 > $OUT/prof_rc.log 2>&1 || exit $?
python scripts/prof_summary.py $OUT/prof_rc/rc_kernel_trace.csv 7 40 > $OUT/prof_rc_summary.txt
python scripts/step_timeline.py $OUT/prof_rc/rc_kernel_trace.csv 1 > $OUT/step_timeline_rc.txt
rm -rf $OUT/prof_att8
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_att8 -o att8 -- python bench.py --steps 5 --warmup 2 --num_chunks 8 > $OUT/prof_att8.log 2>&1 || exit $?
python scripts/prof_summary.py $OUT/prof_att8/att8_kernel_trace.csv 7 40 > $OUT/prof_att8_summary.txt
