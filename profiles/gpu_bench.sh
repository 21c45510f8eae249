# Bench B and C + rocprofv3 kernel-trace summary of config B.
# Run from the repo root: bash profiles/gpu_bench.sh [output directory, default bench_out]
set -o pipefail
O=${1:-bench_out}
mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 300 python bench.py --full > $O/bench_B.json 2> $O/bench_B.err || exit 1
timeout -k 10 300 python bench.py --full --config C --no-cpu-baseline > $O/bench_C.json 2> $O/bench_C.err || exit 1
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof_B -o run -- python bench.py --full --steps 2 --no-cpu-baseline > $O/prof_B.log 2>&1 || exit 1
