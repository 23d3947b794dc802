#!/bin/bash
# GPU box: parity tests (stop at the first failure), then a C3-only bench line (20 and 200 steps).
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-bench_out}; export OUT  # where the logs and result lines go
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread ${PYTEST_K:+-k "$PYTEST_K"} > $OUT/gpu_tests.log 2>&1
rc=$?; tail -15 $OUT/gpu_tests.log; [ $rc = 0 ] || exit $rc
for s in 20 200; do
  timeout -k 10 200 python -u bench.py --full --steps $s --warmup 5 --no-cpu-baseline --no-secondary ${BENCH_EXTRA} > $OUT/bq$s.json 2> $OUT/bq$s.err || { tail -5 $OUT/bq$s.err; exit 1; }
done
python3 - <<'PY'
import json, os
for f in ["bq20", "bq200"]:
    d = json.loads([l for l in open(os.path.join(os.environ["OUT"], f + ".json")) if l.startswith("{")][-1])
    print(f, round(d["value"]), round(d["ms_per_step"], 5), "k_raster", round(d["roofline"]["kernel_ms"], 5), d["stage_ms"])
PY
