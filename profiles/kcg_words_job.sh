#!/bin/bash
# Stored words of the windowed blocked form of K (dkmc_set_k_window_word_bytes): tile:20 and tile:10 with the current off, in one process per step and
# on one box: tools/time_kcg_forms.py plain (windowed 4-byte, CSR positions, windowed 2-byte, windowed 4-byte again: the two 4-byte lines are the
# run-to-run spread of the reference point), then the same script at tile:20 under rocprofv3 --kernel-trace --stats (no counters), from which
# tools/kcg_product_launches.py takes the mean working launch of k_kbw_apply<0, 4> and k_kbw_apply<0, 2> and the rate on their bytes.
# Every GPU step has its own time limit.  Everything it writes goes under OUTPUT_DIR.
set -o pipefail
OUT=${1:?usage: bash profiles/kcg_words_job.sh OUTPUT_DIR}
mkdir -p "$OUT"
timeout -k 10 300 python -c "import __graft_entry__ as g; g.build()" > "$OUT/build.log" 2>&1 || exit 1
timeout -k 10 420 python tools/time_kcg_forms.py tile:20 tile:10 --steps 3 2> "$OUT/kcg_words.err" | tee "$OUT/kcg_words.jsonl" || { tail -20 "$OUT/kcg_words.err"; exit 1; }
timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/rocprof_kcg_tile20" -o kcg -- \
    python tools/time_kcg_forms.py tile:20 --steps 1 > "$OUT/rocprof_kcg_tile20.log" 2>&1 || { tail -20 "$OUT/rocprof_kcg_tile20.log"; exit 1; }
python tools/kcg_product_launches.py "$OUT/rocprof_kcg_tile20" "$OUT/kcg_words.jsonl" tile:20 | tee "$OUT/kcg_words_tile20_product_launches.txt"
