#!/bin/bash
# K-CG on the CSR positions against the windowed blocked form (dkmc_set_k_blocked_large), tile:20 and tile:10 with the current off:
# tools/time_kcg_forms.py plain (iterations, loop time per iteration, superstep rate, window statistics), then the same script at tile:20
# under rocprofv3 --kernel-trace --stats (mean launch time of k_kc_apply against k_kbw_apply).  Every GPU step has its own time limit.
# Everything it writes goes under OUTPUT_DIR.
set -o pipefail
OUT=${1:?usage: bash profiles/kcg_forms_job.sh OUTPUT_DIR}
mkdir -p "$OUT"
timeout -k 10 300 python -c "import __graft_entry__ as g; g.build()" > "$OUT/build.log" 2>&1 || exit 1
timeout -k 10 420 python tools/time_kcg_forms.py tile:20 tile:10 --steps 3 2> "$OUT/kcg_forms.err" | tee "$OUT/kcg_forms.jsonl" || { tail -20 "$OUT/kcg_forms.err"; exit 1; }
timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/rocprof_kcg_tile20" -o kcg -- \
    python tools/time_kcg_forms.py tile:20 --steps 1 > "$OUT/rocprof_kcg_tile20.log" 2>&1 || { tail -20 "$OUT/rocprof_kcg_tile20.log"; exit 1; }
find "$OUT/rocprof_kcg_tile20" -name "*kernel_stats.csv" -exec grep -h "Name\|k_kc_apply\|k_kbw_apply\|k_kc_update\|k_kc_direction" {} \;
