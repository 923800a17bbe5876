# the whole GPU suite, then the full bench line (bench.py --full); outputs under $OUT (default out/)
set -o pipefail
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT=${OUT:-out}
mkdir -p $OUT
timeout -k 10 1050 python -u -m pytest tests -x -v -m gpu --timeout 400 --timeout-method thread > $OUT/pytest_gpu.log 2>&1 || { echo PYTEST_FAIL; tail -30 $OUT/pytest_gpu.log; exit 1; }
tail -3 $OUT/pytest_gpu.log
[ -n "$NO_BENCH" ] || timeout -k 10 600 python bench.py --full --steps 10 --warmup 2 > $OUT/bench.json 2> $OUT/bench.err || { echo BENCH_FAIL; tail -20 $OUT/bench.err; exit 1; }
[ -n "$NO_BENCH" ] || cat $OUT/bench.json
