# k_recon tuning sweep on the GPU box: bench.py under each value of a
# THOR_RECON_* environment knob (usage: sweep_recon.sh VAR v1 v2 ...)
set -o pipefail
cd /root/repo
OUT=${OUT:-out}/sweep
mkdir -p $OUT
var=$1; shift
for w in "$@"; do
  env $var=$w timeout -k 10 120 python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-legs --no-rows > $OUT/$var.$w.json 2> $OUT/$var.$w.err || { echo FAIL $w; tail -5 $OUT/$var.$w.err; exit 1; }
  python -c "import json;d=json.load(open('$OUT/$var.$w.json'));print('$var', $w, d['value'], d['ms_per_step'], d['roofline']['avg_launch_us'], d['roofline']['frac'])"
done
