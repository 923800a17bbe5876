# Round-end evidence on the box: the full bench line (bench.py --full: legs, CPU baseline, rows), then the bench
# under rocprofv3 --kernel-trace --stats and the decoder FETCH / WRITE passes (tools/profile_round.sh).
# Usage: bash tools/gpu_final.sh TAG   (outputs under $OUT/TAG and $OUT/prof; OUT defaults to out)
set -o pipefail
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
TAG=${1:-final}
export OUT=${OUT:-out}
mkdir -p $OUT/$TAG
timeout -k 10 700 python bench.py --full --steps 5 --warmup 1 > $OUT/$TAG/bench.json 2> $OUT/$TAG/bench.err || { echo BENCH_FAIL; tail -20 $OUT/$TAG/bench.err; exit 1; }
tail -c 600 $OUT/$TAG/bench.json
[ -n "$WITH_PROFILE" ] || { echo FINAL_OK; exit 0; }
timeout -k 10 700 bash tools/profile_round.sh > $OUT/$TAG/profile.log 2>&1 || { echo PROFILE_FAIL; tail -20 $OUT/$TAG/profile.log; exit 1; }
echo FINAL_OK
