#!/bin/bash
# The variance-guided denoiser's per-kernel device times against the plain filter's on C3's frame (GPU box, repo
# root): tools/gpu/denoise_guided_cost.py under rocprofv3's kernel trace (a run of its own, no counters), then
# tools/gpu/denoise_guided_cost_report.py.  Output in ${OUT_DIR:-bench_out}/${TAG:-denoise_guided_cost}:
# denoise_guided_cost.json (the table), run.json (the script's own line) and the trace's kernel_stats.csv.  Stops at
# the first failure.
set -o pipefail
export TMPDIR=/tmp
OUT=${OUT_DIR:-bench_out}/${TAG:-denoise_guided_cost}
mkdir -p $OUT
timeout -k 10 ${TLIM:-300} rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/ktrace -o run -- \
    python3 tools/gpu/denoise_guided_cost.py > $OUT/run.json 2> $OUT/run.err \
    || { echo "denoise-guided-cost-fail" > $OUT/done.txt; tail -5 $OUT/run.err; exit 1; }
TRACE=$(find $OUT/ktrace -name run_kernel_trace.csv | head -1)
STATS=$(find $OUT/ktrace -name run_kernel_stats.csv | head -1)
python3 tools/gpu/denoise_guided_cost_report.py "$TRACE" > $OUT/denoise_guided_cost.json || { echo "report-fail" > $OUT/done.txt; exit 1; }
cp "$STATS" $OUT/kernel_stats.csv
rm -rf $OUT/ktrace
echo ok > $OUT/done.txt
cat $OUT/run.json
