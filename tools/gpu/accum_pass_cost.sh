#!/bin/bash
# The cost of resumable accumulation on C3 (GPU box, repo root): tools/gpu/accum_pass_cost.py under its own
# time limit; the JSON goes to ${OUT_DIR:-bench_out}/${TAG:-accum_cost}/accum_pass_cost.json.  Stops at the first failure.
set -o pipefail
export TMPDIR=/tmp
OUT=${OUT_DIR:-bench_out}/${TAG:-accum_cost}
mkdir -p $OUT
timeout -k 10 ${TLIM:-240} python3 tools/gpu/accum_pass_cost.py > $OUT/accum_pass_cost.json 2> $OUT/accum_pass_cost.err \
    || { echo "accum-cost-fail" > $OUT/done.txt; tail -5 $OUT/accum_pass_cost.err; exit 1; }
echo ok > $OUT/done.txt
