#!/bin/bash
# Round-end rehearsal (GPU box, repo root): the whole GPU suite, smoke(), the default bench with
# everything it measures (--full).  Logs go to $OUT (default build/check, which git ignores).
set -e
O=${OUT:-build/check}
mkdir -p $O
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > $O/full_tests.log 2>&1
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $O/full_smoke.log 2>&1
timeout -k 10 600 python3 bench.py --full > $O/full_bench.log 2>&1
# the shared-policy lines (C4 SharedDecentral, C5 Graph at 2048 envs), one iteration each
timeout -k 10 300 python3 bench.py --env QuantrupedMultiEnv_SharedDecentral --steps 1 --warmup 1 > $O/full_bench_c4.log 2>&1
timeout -k 10 300 python3 bench.py --env QuantrupedMultiEnv_DecentralShared_Graph --envs 2048 --steps 1 --warmup 1 > $O/full_bench_c5.log 2>&1
