# The hashed-grid GPU tests, then the full bench line's hashed_grid and reference_mode figures.
#   tools/gpu_hash_check.sh OUTDIR
set -u
OUT="${1:?usage: tools/gpu_hash_check.sh OUTDIR}"
cd $GRAFT_REPO_ROOT
mkdir -p "$OUT"
export HSA_ENABLE_IPC_MODE_LEGACY=0
timeout -k 10 600 python -u -m pytest tests/test_gpu_hash.py -x -v --timeout 300 --timeout-method thread > "$OUT/tests.log" 2>&1; rc=$?
tail -25 "$OUT/tests.log"
[ $rc -lt 124 ] || exit $rc
timeout -k 10 600 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > "$OUT/bench.log" 2>&1; rc=$?
tail -1 "$OUT/bench.log" | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print(d['value'], d['hashed_grid'], d['reference_mode'])"
exit $rc
