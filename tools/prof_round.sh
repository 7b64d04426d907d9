#!/bin/bash
# usage: tools/prof_round.sh <tag> [bench args]     default bench args = the driver's: --gpus 1 --steps 20 --warmup 5
# 1. kernel trace + stats of that bench command   2. HBM traffic counters (one --pmc pass per counter, kept apart from the trace pass)
# -> build/prof_<tag>_*, condensed by prof_summary.py into profiles/<tag>_*.  Stops at the first pass that fails or times out.
tag=$1; shift
ARGS=${@:-"--gpus 1 --steps 20 --warmup 5"}
R=$(cd "$(dirname "$0")/.." && pwd)
fail() { echo "$1 failed (exit $2)"; exit "$2"; }
rm -rf "$R"/build/prof_${tag}_trace "$R"/build/prof_${tag}_FETCH_SIZE "$R"/build/prof_${tag}_WRITE_SIZE      # (stale runs would be counted twice)
mkdir -p "$R"/build
cd /tmp && export TMPDIR=/tmp
timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $R/build/prof_${tag}_trace -- python3 $R/bench.py $ARGS --no-cpu-baseline --no-boundary-leg > $R/build/prof_${tag}_trace.log 2>&1 || fail "trace pass" $?
for c in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 500 rocprofv3 --pmc $c --kernel-trace --output-format csv -d $R/build/prof_${tag}_$c -- python3 $R/bench.py $ARGS --no-cpu-baseline --no-boundary-leg --launch eager > $R/build/prof_${tag}_$c.log 2>&1 || fail "$c pass" $?
done
cd "$R" && python3 tools/prof_summary.py $tag "$ARGS"
