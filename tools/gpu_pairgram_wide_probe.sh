#!/bin/bash
# One GPU-box session of tools/pairgram_wide_probe.py: the small-shape checks, the timing run,
# the stage table of the whole calls, and one FETCH_SIZE counter pass (a run of its own, no
# tracing flags).  Every GPU step has its own time limit and the chain stops at the first failure.
# usage: tools/gpu_pairgram_wide_probe.sh [OUT_DIR]   (default check_out/, which git ignores;
#        the result is OUT_DIR/pairgram_wide_probe.json, to be copied to profiles/)
set -o pipefail
OUT=${1:-check_out}
mkdir -p "$OUT"
J="$OUT"/pairgram_wide_probe.json
P=tools/pairgram_wide_probe.py
timeout -k 10 180 python -u $P --step check --out "$J" > "$OUT"/pairgram_wide_check.log 2>&1 \
 && timeout -k 10 420 python -u $P --step time --out "$J" > "$OUT"/pairgram_wide_time.log 2>&1 \
 && timeout -k 10 420 python -u $P --step stages --out "$J" > "$OUT"/pairgram_wide_stages.log 2>&1 \
 && timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$OUT"/pairgram_wide_pmc -o b \
      -- python -u $P --step pmc_run > "$OUT"/pairgram_wide_pmc.log 2>&1 \
 && CSV=$(find "$OUT"/pairgram_wide_pmc -name '*counter_collection.csv' | head -1) \
 && python -u $P --step pmc_read --csv "$CSV" --out "$J" > "$OUT"/pairgram_wide_pmc_read.log 2>&1
rc=$?
for s in check time stages pmc pmc_read; do echo "== $s"; tail -8 "$OUT"/pairgram_wide_$s.log 2>/dev/null; done
exit $rc
