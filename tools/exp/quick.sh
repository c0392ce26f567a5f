# quick check: parity tests (optional), one bench line, kernel averages from rocprofv3
set -u
cd "$(dirname "$0")/../.."; export OUT_DIR=${OUT_DIR:-bench_out}; mkdir -p $OUT_DIR; export TMPDIR=/tmp
if [ "${TESTS:-1}" = 1 ]; then
  timeout -k 10 300 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT_DIR/pytest_gpu.log 2>&1; rc=$?; tail -2 $OUT_DIR/pytest_gpu.log; [ $rc -eq 0 ] || exit $rc
fi
timeout -k 10 300 python bench.py --full --steps 50 --warmup 5 --cpu-baseline 0 ${BENCH_ARGS:-} > $OUT_DIR/bench.log 2>&1 || exit $?
python -c "import json;d=json.loads(open('$OUT_DIR/bench.log').read().strip().splitlines()[-1]);print(round(d['value'],1),d['parity_vs_oracle'],{k:round(v*1000,1) for k,v in d['stages_ms'].items()})"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT_DIR/prof -o run -- python bench.py --full --steps 20 --warmup 3 --cpu-baseline 0 --parity 0 ${BENCH_ARGS:-} > $OUT_DIR/rocprof.log 2>&1 || exit $?
python - <<'PY'
import csv, glob, os
f = glob.glob(os.environ['OUT_DIR'] + '/prof/**/*kernel_stats.csv', recursive=True)[0]
tot = 0
for r in csv.DictReader(open(f)):
    print(r['Name'][:60].ljust(60), r['Calls'].rjust(4), round(float(r['AverageNs'])/1000, 1))
PY
