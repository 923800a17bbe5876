# quick GPU check: stream parity tests + a short bench (no CPU baseline); outputs under $OUT (default out/)
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-out}
mkdir -p $OUT
timeout -k 10 300 python -u -m pytest tests/test_gpu_streams.py tests/test_synth_frames.py -x -q -m gpu --timeout 120 --timeout-method thread > $OUT/quick_pytest.log 2>&1 || { echo PYTEST_FAIL; tail -30 $OUT/quick_pytest.log; exit 1; }
tail -2 $OUT/quick_pytest.log
timeout -k 10 300 python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-legs --no-rows > $OUT/quick_bench.json 2> $OUT/quick_bench.err || { echo BENCH_FAIL; tail -20 $OUT/quick_bench.err; exit 1; }
python -c "import json;d=json.load(open('$OUT/quick_bench.json'));print(d['value'], d['ms_per_step'], d['roofline']['avg_launch_us'], d['roofline']['frac'])"
