# GPU box: every gpu test, smoke, the driver-shaped bench, the owner-path bench, kernel-trace profiles of both.
# Usage: bash scripts/gpu_full.sh TAG      (from the repository root; results under $OUT, default out/)
set -o pipefail
TAG=${1:-run}
R=$(pwd)
OUT=${OUT:-out}
mkdir -p $OUT && OUT=$(cd $OUT && pwd) || exit 1
export TMPDIR=/tmp
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread -p no:cacheprovider > $OUT/gpu_tests_$TAG.log 2>&1
rc=$?; echo "tests exit=$rc"; tail -4 $OUT/gpu_tests_$TAG.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$TAG.log 2>&1 || exit $?
echo smoke-ok
timeout -k 10 300 python3 bench.py --gpus 1 --steps 20 --warmup 5 --full --no-cpu-baseline > $OUT/bench20_$TAG.json 2>$OUT/bench20_$TAG.err || exit $?
python -c "import json;d=json.load(open('$OUT/bench20_$TAG.json'));print('b20', d['value']/1e6, d['ms_per_step'], d['roofline']['avg_launch_us'], d['plan_build_us_per_batch'])"
timeout -k 10 300 python3 bench.py --gpus 1 --steps 50 --warmup 5 --dp owner --dp-at-1 > $OUT/bench_own_$TAG.json 2>$OUT/bench_own_$TAG.err || exit $?
python -c "import json;d=json.load(open('$OUT/bench_own_$TAG.json'));print('own', d['value']/1e6, d['ms_per_step'], d['roofline']['avg_launch_us'])"
# the profiler writes its scratch files into the working directory: run it from a temporary one
T=$(mktemp -d) && cd $T || exit 1
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o run -- python3 $R/bench.py --steps 20 --warmup 5 > $OUT/prof_bench_$TAG.json 2>$OUT/prof_$TAG.err || exit $?
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_own_$TAG -o run -- python3 $R/bench.py --steps 20 --warmup 5 --dp owner --dp-at-1 > $OUT/prof_own_bench_$TAG.json 2>$OUT/prof_own_$TAG.err && echo prof-ok
