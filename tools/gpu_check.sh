#!/bin/bash
# One GPU-box session: parity tests, smoke, bench (--full: with the CPU baseline), rocprofv3 kernel stats.
# Every GPU step has its own time limit and the chain stops at the first failure.
# usage: tools/gpu_check.sh [TAG] [OUT_DIR]   (OUT_DIR defaults to check_out/, which git ignores)
set -o pipefail
TAG=${1:-r01}
OUT=${2:-check_out}
mkdir -p "$OUT"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread> "$OUT"/pytest_gpu_${TAG}.log 2>&1 \
 && timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT"/smoke_${TAG}.log 2>&1 \
 && timeout -k 10 600 python bench.py --full > "$OUT"/bench_${TAG}.json 2> "$OUT"/bench_${TAG}.err \
 && cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT" \
 && timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT"/prof_${TAG} -o bench \
      -- python3 bench.py --steps 20 > "$OUT"/prof_${TAG}.log 2>&1
rc=$?
tail -3 "$OUT"/pytest_gpu_${TAG}.log; cat "$OUT"/smoke_${TAG}.log 2>/dev/null; cat "$OUT"/bench_${TAG}.json 2>/dev/null
exit $rc
