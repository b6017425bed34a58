#!/bin/bash
# Planner prefix sums with the u32 list-length table: C3 kernel stats, the bench line, then the whole GPU suite.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
ROOT=$(pwd)
OUT=${OUT:-bench_out}  # results, relative to the repository root
mkdir -p $OUT/scan3
export TMPDIR=/tmp
(cd /tmp && timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$ROOT/$OUT/scan3/prof_c3" -o run --output-format csv \
  -- python3 "$ROOT/bench.py" --config c3 --steps 3 --warmup 1 --no-cpu-baseline > "$ROOT/$OUT/scan3/prof_c3.log" 2>&1) || exit 1
echo "prof ok"
timeout -k 10 600 python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline > $OUT/scan3/bench.json 2> $OUT/scan3/bench.err || exit 1
python -c "import json; d=json.load(open('$OUT/scan3/bench.json')); print('c3', d['value'], d['ms_per_step'], d['roofline']['kernel_ms'], d['roofline']['frac'], d.get('permuted', {}).get('ms_per_step'))"
timeout -k 10 900 python -u -m pytest tests -m gpu -q -x --timeout 300 --timeout-method thread > $OUT/scan3/pytest_gpu.log 2>&1
rc=$?; tail -3 $OUT/scan3/pytest_gpu.log; exit $rc
