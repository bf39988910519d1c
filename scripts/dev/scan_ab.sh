# Development: A/B of library variants (varlib/<name>) on the config-3 scans, alternating, twice.
# Usage (on the GPU box): VARIANTS="head other" bash scripts/dev/scan_ab.sh
set -o pipefail
cd "${GRAFT_REPO_ROOT:-.}" || exit 1
OUT=${OUT:-bench_out}/scan_ab
mkdir -p "$OUT"
for rep in 1 2; do for v in ${VARIANTS:-head}; do
  SGXAMD_LIB_PATH=$PWD/varlib/$v/libsgxamd.so timeout -k 10 300 python bench.py --full --steps 2 --warmup 1 --no-tpch --no-cpu-baseline --no-paper --no-configs --no-tuple-layout > "$OUT/$v.$rep.json" 2> "$OUT/$v.$rep.err" || { tail -5 "$OUT/$v.$rep.err"; exit 1; }
  python3 -c "
import json; s=json.load(open('$OUT/$v.$rep.json'))['scan']
print('$v', $rep, s['count']['kernel_ms_avg'], s['bitvector']['kernel_ms_avg'], s['index']['kernel_ms_avg'])"
done; done
