set -o pipefail
export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 600 python -m pytest tests -m gpu -q -p no:cacheprovider > "$OUT/gpu_tests_4.log" 2>&1 || { echo "pytest failed"; tail -30 "$OUT/gpu_tests_4.log"; exit 1; }
tail -3 "$OUT/gpu_tests_4.log"
timeout -k 10 600 python bench.py --full --steps 10 --warmup 3 > "$OUT/bench_1.json" 2> "$OUT/bench_1.err" || { echo "bench failed"; tail -30 "$OUT/bench_1.err"; exit 1; }
cat "$OUT/bench_1.json"
lscpu > "$OUT/lscpu.txt"; nproc >> "$OUT/lscpu.txt"
