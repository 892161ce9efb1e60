set -o pipefail
OUT=${OUT:-verify_out}
mkdir -p "$OUT"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > "$OUT/pytest_gpu.log" 2>&1 && \
timeout -k 10 180 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1 && \
timeout -k 10 180 python bench.py --full > "$OUT/bench.log" 2>&1
echo "rc=$?"; tail -3 "$OUT/pytest_gpu.log"; cat "$OUT/bench.log"
