#!/bin/bash
# Rollout forward with its input loads ahead of the weight staging: GPU suite, kernel trace
# of the Local bench, default bench.  Logs go to $OUT (default build/act, which git ignores).
set -e
R=$(pwd)
A=$R/${OUT:-build/act}
mkdir -p $A
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > $A/tests.log 2>&1
cd /tmp && export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_local -o run -- python3 $R/bench.py --steps 2 --warmup 1 > $A/trace_local.log 2>&1
cp /tmp/prof_local/run_kernel_stats.csv $A/local_kernel_stats.csv
cd $R
timeout -k 10 400 python3 bench.py --full > $A/bench.log 2>&1
