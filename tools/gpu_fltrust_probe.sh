#!/bin/bash
# One GPU-box session of tools/fltrust_probe.py: the small-shape checks, then the timing run.
# Every GPU step has its own time limit and the chain stops at the first failure.  The two batch
# builds of dotnorm2_kernel must exist already (python tools/fltrust_probe.py --step build, where
# the compiler is).
# usage: tools/gpu_fltrust_probe.sh [OUT_DIR]   (default check_out/, which git ignores;
#        the result is OUT_DIR/fltrust_probe.json, to be copied to profiles/)
set -o pipefail
OUT=${1:-check_out}
mkdir -p "$OUT"
J="$OUT"/fltrust_probe.json
P=tools/fltrust_probe.py
timeout -k 10 180 python -u $P --step check --out "$J" > "$OUT"/fltrust_check.log 2>&1 \
 && timeout -k 10 300 python -u $P --step time --out "$J" > "$OUT"/fltrust_time.log 2>&1
rc=$?
for s in check time; do echo "== $s"; tail -8 "$OUT"/fltrust_$s.log 2>/dev/null; done
exit $rc
