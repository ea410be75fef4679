#!/bin/bash
# What a checkpoint and a session file cost on C3's frame (GPU box, repo root): tools/gpu/session_cost.py once with the
# profiler off (the stage times) and once under rocprofv3's kernel trace (a run of its own, no counters, fewer
# repeats: the pack / unpack kernels' device times), then its --report.  Output in
# ${OUT_DIR:-bench_out}/${TAG:-session_cost}: session_cost.json (the table), run.json / trace_run.json (the script's
# own lines) and the trace's kernel_stats.csv.  Stops at the first failure.
set -o pipefail
export TMPDIR=/tmp
OUT=${OUT_DIR:-bench_out}/${TAG:-session_cost}
mkdir -p $OUT
timeout -k 10 ${TLIM:-300} python3 tools/gpu/session_cost.py > $OUT/run.json 2> $OUT/run.err \
    || { echo "session-cost-fail" > $OUT/done.txt; tail -5 $OUT/run.err; exit 1; }
REPS=3 timeout -k 10 ${TLIM:-300} rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/ktrace -o run -- \
    python3 tools/gpu/session_cost.py > $OUT/trace_run.json 2> $OUT/trace_run.err \
    || { echo "session-trace-fail" > $OUT/done.txt; tail -5 $OUT/trace_run.err; exit 1; }
TRACE=$(find $OUT/ktrace -name run_kernel_trace.csv | head -1)
STATS=$(find $OUT/ktrace -name run_kernel_stats.csv | head -1)
python3 tools/gpu/session_cost.py --report $OUT/run.json > $OUT/session_cost.json || { echo "report-fail" > $OUT/done.txt; exit 1; }
python3 tools/gpu/session_cost.py --report $OUT/trace_run.json "$TRACE" > $OUT/session_cost_traced.json || { echo "report-fail" > $OUT/done.txt; exit 1; }
cp "$STATS" $OUT/kernel_stats.csv
rm -rf $OUT/ktrace
echo ok > $OUT/done.txt
cat $OUT/session_cost.json
python3 -c "import json,sys; print(json.dumps(json.load(open(sys.argv[1]))['kernels'], indent=1))" $OUT/session_cost_traced.json
