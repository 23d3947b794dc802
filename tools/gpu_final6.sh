#!/bin/bash
# Round-6 closing session on one GPU box: the GPU suite, the driver-shaped bench line (20 steps, and 200 for the
# steady state), then rocprofv3 kernel traces + PMC passes for C3 and C5 (tools/profile.sh). Every GPU step has its own
# time limit and the chain stops at the first failure.
OUT=${OUT:-bench_out}; export OUT  # where the logs and result lines go
cd "$(dirname "$0")/.." && mkdir -p $OUT && export TMPDIR=/tmp
timeout -k 10 420 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread > $OUT/gpu_tests.log 2>&1 \
  || { tail -5 $OUT/gpu_tests.log; grep -E "FAILED|Error" $OUT/gpu_tests.log | head; exit 1; }
tail -1 $OUT/gpu_tests.log
timeout -k 10 400 python bench.py --full --steps 20 > $OUT/bench.json 2> $OUT/bench.err || { tail -5 $OUT/bench.err; exit 1; }
timeout -k 10 300 python bench.py --full --steps 200 --no-cpu-baseline --no-secondary > $OUT/bench200.json 2> $OUT/bench200.err || { tail -5 $OUT/bench200.err; exit 1; }
echo bench ok
PROF_OUT=$OUT/prof_c3 bash tools/profile.sh > $OUT/prof_c3.log 2>&1 || { tail -5 $OUT/prof_c3.log; exit 1; }
PROF_OUT=$OUT/prof_c5 BENCH_ARGS="--config c5 --steps 50 --warmup 5 --no-cpu-baseline --no-secondary --inflight 1" \
  bash tools/profile.sh > $OUT/prof_c5.log 2>&1 || { tail -5 $OUT/prof_c5.log; exit 1; }
echo prof ok
# N = 8 per-rank rates on this GPU (assemble-only display: rank 0 decodes the seven bands; senders 1, 4, 7)
DROWS=0 RANKS="0 1 4 7" timeout -k 10 900 bash tools/sim_split.sh > $OUT/sim_split6.txt 2>&1 || { tail -5 $OUT/sim_split6.txt; exit 1; }
cat $OUT/sim_split6.txt
