set -o pipefail
OUT=${OUT:-bench_out}  # results, relative to the repository root
mkdir -p $OUT
for v in new head new head; do
  if [ $v = head ]; then export COOC_LIB=flink-cooccurrence_amd/csrc/libcooc_hip_head.so; else unset COOC_LIB; fi
  timeout -k 10 300 python -u bench.py --full --config c5 --steps 3 --warmup 1 --no-cpu-baseline > $OUT/c5_$v.json 2> $OUT/c5_$v.err || { echo "bench $v failed"; tail -5 $OUT/c5_$v.err; exit 1; }
  python -c "import json;d=json.load(open('$OUT/c5_$v.json'));r=d.get('roofline_rescore',{});print('$v', 'ms', d['ms_per_step'], 'rescore', {k:r.get(k) for k in ('kernel_ms','achieved','frac')})"
done
unset COOC_LIB
timeout -k 10 900 python -u -m pytest tests/test_gpu_exactness.py tests/test_gpu_parity.py tests/test_gpu_configs.py tests/test_owned_operator_replay.py -m gpu -x -q --timeout 600 > $OUT/c5_tests.log 2>&1; rc=$?; tail -3 $OUT/c5_tests.log; exit $rc
