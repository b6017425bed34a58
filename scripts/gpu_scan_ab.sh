#!/bin/bash
# Hand-written planner prefix sums (cooc_scan.h): the GPU suite, the C3 bench line and its kernel stats.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
ROOT=$(pwd)
OUT=${OUT:-bench_out}  # results, relative to the repository root
mkdir -p $OUT/scan
if [ "${SKIP_TESTS:-0}" != "1" ]; then
  timeout -k 10 900 python -u -m pytest tests -m gpu -q -x --timeout 300 --timeout-method thread > $OUT/scan/pytest_gpu.log 2>&1
  rc=$?; tail -3 $OUT/scan/pytest_gpu.log; [ $rc -eq 0 ] || exit $rc
fi
timeout -k 10 600 python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline > $OUT/scan/bench.json 2> $OUT/scan/bench.err || exit 1
python -c "import json; d=json.load(open('$OUT/scan/bench.json')); print('c3', d['value'], d['ms_per_step'], d['roofline']['kernel_ms'], d['roofline']['frac'], d.get('permuted', {}).get('ms_per_step'))"
export TMPDIR=/tmp
cd /tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$ROOT/$OUT/scan/prof_c3" -o run --output-format csv \
  -- python3 "$ROOT/bench.py" --config c3 --steps 3 --warmup 1 --no-cpu-baseline > "$ROOT/$OUT/scan/prof_c3.log" 2>&1 || exit 1
echo done
