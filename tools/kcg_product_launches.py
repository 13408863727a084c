#!/usr/bin/env python3
"""Per-launch times of the K-CG's kernels from a rocprofv3 --kernel-trace run of tools/time_kcg_forms.py, and for the windowed products the bytes a launch
moves (from that script's own json lines: stored words x word bytes + window copies + block records and segment tables + 5 vector touches) and the
rate on those bytes.  Launches of at most 10 us are the no-op tails after the stop test of a launch batch: counted, not averaged.
usage: python tools/kcg_product_launches.py TRACE_DIR FORMS.jsonl [workload]"""
import collections
import csv
import glob
import json
import os
import sys

KERNELS = ("k_kc_apply<0>", "k_kbw_apply<0, 4>", "k_kbw_apply<0, 2>", "k_kc_update", "k_kc_direction", "k_kc_assemble<0>", "k_kbw_assemble<0, 4>", "k_kbw_assemble<0, 2>")


def main():
    trace_dir, forms = sys.argv[1], sys.argv[2]
    workload = sys.argv[3] if len(sys.argv) > 3 else "tile:20"
    dur = collections.defaultdict(list)
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"].split("(")[0].replace("void ", "").strip()
            dur[name].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    mean = {}
    for k in KERNELS:
        d = dur.get(k, [])
        w = [x for x in d if x > 10.0]
        mean[k] = sum(w) / len(w) if w else 0.0
        print("%-22s launches %6d working %6d mean working %8.1f us" % (k, len(d), len(w), mean[k]))
    for line in open(forms):
        r = json.loads(line)
        if r.get("workload") != workload or r.get("form") != 2:
            continue
        wb, k = r["word_bytes"], "k_kbw_apply<0, %d>" % r["word_bytes"]
        words, win = r["stored_ints"] * wb, r["blocks"] * r["window_mean"] * 8
        tabs, vec = r["blocks"] * 17 * 16, 5 * 8 * r["K_rows"]
        tot = words + win + tabs + vec
        print("%s %s: words %.1f MB + windows %.1f MB + tables %.1f MB + vectors %.1f MB = %.1f MB per launch; %.1f us -> %.2f TB/s; %.2f us per iteration, %.3f supersteps/s"
              % (workload, k, words / 1e6, win / 1e6, tabs / 1e6, vec / 1e6, tot / 1e6, mean[k], tot / mean[k] / 1e6 if mean[k] else 0.0, r["us_per_iter"], r["steps_per_s"]))


if __name__ == "__main__":
    main()
