#!/bin/bash
# One GPU-box session of tools/trimmed_wide_probe.py: the bit-for-bit checks, a small
# timing run, the full timing run and the config-4 launch.  Every GPU step has its own
# time limit and the chain stops at the first failure.  The full run's limit follows from
# the seconds the small run's torch legs took (1/16 of the columns, 3 rounds against 11),
# three times over, plus two minutes for making the rows.
# usage: tools/gpu_trimmed_wide_probe.sh [OUT_DIR]   (default check_out/, which git ignores;
#        the result is OUT_DIR/trimmed_wide_probe.json, to be copied to profiles/)
set -o pipefail
OUT=${1:-check_out}
mkdir -p "$OUT"
J="$OUT"/trimmed_wide_probe.json
timeout -k 10 300 python -u tools/trimmed_wide_probe.py --step check --out "$J" > "$OUT"/trimmed_wide_check.log 2>&1 \
 && cp "$J" "$OUT"/trimmed_wide_small.json \
 && timeout -k 10 300 python -u tools/trimmed_wide_probe.py --step time --cols 262144 --iters 2 \
      --out "$OUT"/trimmed_wide_small.json > "$OUT"/trimmed_wide_small.log 2>&1 \
 && LIMIT=$(python -c "import json,sys; s=json.load(open(sys.argv[1]))['torch_leg_seconds_total']; print(int(120 + 3 * s * 16 * 11 / 3))" "$OUT"/trimmed_wide_small.json) \
 && echo "full timing run: limit ${LIMIT}s" \
 && timeout -k 10 "$LIMIT" python -u tools/trimmed_wide_probe.py --step time --out "$J" > "$OUT"/trimmed_wide_time.log 2>&1 \
 && timeout -k 10 300 python -u tools/trimmed_wide_probe.py --step config4 --out "$J" > "$OUT"/trimmed_wide_config4.log 2>&1
rc=$?
tail -2 "$OUT"/trimmed_wide_check.log; tail -1 "$OUT"/trimmed_wide_small.log
tail -1 "$OUT"/trimmed_wide_time.log 2>/dev/null; tail -1 "$OUT"/trimmed_wide_config4.log 2>/dev/null
exit $rc
