#!/usr/bin/env python3
"""The size gate of the live view's auto mode (dkmc_set_x_tile_drop_auto; csrc/xt_live.h: xtl_drop_rule), measured on whole supersteps.  One child
process per workload, each under its own time limit; in it, after one short discarded case (the first device of a process runs slower: it grows the
allocator's pools), the cases theta = 0, 1e-10, 0, 1e-10, 0 run one after the other (tools/time_tile_drop.py:
run -- a fresh device with the same seeds per case, `warmup` untimed supersteps, then the timed ones, all warm-started).  The three theta = 0 cases
are the reference point: their median and their spread (max - min) / median.  A size GAINS when the median rate of its two theta = 1e-10 cases exceeds
the reference median by more than 3 x that spread (the project's rule).  The gate is the geometric midpoint, in stored sub-blocks, between the largest
size that does not gain and the smallest that does.

Written to <out-dir>/x_tile_drop_by_size.jsonl: one line per case, one verdict line per workload (key `gains`; tests/test_x_tile_drop_rule.py reads
those) and one closing line with the gate (key `gate_subblocks`; no `gains` key).
--pool SERIES ...: no run; the case lines of several such files (one per job) are pooled and the verdicts taken over all their cases.
usage: python tools/x_tile_drop_by_size.py [7.5nm=200 tile:5=30 tile:7=12 tile:10=8] [--warmup 2] [--limit 420] [--out-dir profiles]
       (workload=timed steps; small workloads need more steps for a steady rate)"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CASES = (0.0, 1e-10, 0.0, 1e-10, 0.0)
DEFAULT = ["7.5nm=200", "tile:5=30", "tile:7=12", "tile:10=8"]


def child(name, steps, warmup, path):
    import time_tile_drop
    from devicekmc_amd import host
    # the first device of a process grows the allocator's pools and the library's scratch: its case runs 6-9 % slower at tile:10 whatever its threshold
    # (DESIGN.md section 6), which would count as spread of the reference point -- one short case is run first and discarded
    time_tile_drop.run(name, 0.0, 2, warmup)
    with open(path, "w") as f:
        for theta in CASES:
            rec, _ = time_tile_drop.run(name, theta, steps, warmup)
            rec["stored_subblocks"] = int(host.get_stats()["xt_subblocks"])
            f.write(json.dumps(rec) + "\n"); f.flush()
            print(json.dumps(rec), flush=True)


def verdict(recs):
    ref = [r["steps_per_s"] for r in recs if r["theta"] == 0.0]
    drop = [r["steps_per_s"] for r in recs if r["theta"] > 0.0]
    med = statistics.median(ref); spread = (max(ref) - min(ref)) / med
    got = statistics.median(drop)
    return dict(workload=recs[0]["workload"], sites=recs[0]["sites"], stored_subblocks=recs[0]["stored_subblocks"], theta=max(r["theta"] for r in recs),
                steps_per_s_full_median=round(med, 4), spread_full=round(spread, 5), steps_per_s_live_median=round(got, 4), ratio=round(got / med, 4),
                gains=bool(got > med * (1.0 + 3.0 * spread)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=DEFAULT)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=420, help="time limit of one workload's process, seconds")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--pool", nargs="+", default=None, metavar="SERIES", help="no run: pool the case lines of these series files (one per job) into <out-dir>/x_tile_drop_by_size.jsonl; "
                    "the verdict of a size is then taken over the cases of all series, so it has to hold from job to job")
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], int(a.child[1]), a.warmup, a.child[2])
    os.makedirs(a.out_dir, exist_ok=True)
    lines, verdicts = [], []
    if a.pool:
        by = {}
        for k, path in enumerate(a.pool):
            for r in (json.loads(x) for x in open(path) if x.strip()):
                if "steps_per_s" in r and "info8" in r:
                    r["series"] = k + 1
                    by.setdefault(r["workload"], []).append(r)
        for recs in by.values():
            lines += recs; verdicts.append(dict(verdict(recs), series_pooled=len(a.pool))); lines.append(verdicts[-1])
            print(json.dumps(verdicts[-1]), flush=True)
    for w in ([] if a.pool else a.workloads):
        name, _, steps = w.partition("=")
        part = os.path.join(a.out_dir, "x_tile_drop_by_size_%s.part" % name.replace(":", ""))
        try:
            rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--child", name, steps or "8", part, "--warmup", str(a.warmup)], timeout=a.limit)
        except subprocess.TimeoutExpired:
            rc = 124
        if rc:
            print("%s: child ended with %d" % (name, rc), file=sys.stderr)
            sys.exit(1)               # nothing more is started on the GPU after a failure
        recs = [json.loads(x) for x in open(part)]
        os.remove(part)
        lines += recs; verdicts.append(verdict(recs)); lines.append(verdicts[-1])
        print(json.dumps(verdicts[-1]), flush=True)
    verdicts.sort(key=lambda v: v["stored_subblocks"])
    no = [v["stored_subblocks"] for v in verdicts if not v["gains"]]
    yes = [v["stored_subblocks"] for v in verdicts if v["gains"]]
    if no and yes and max(no) < min(yes):
        gate = dict(gate_subblocks=int(round(math.sqrt(max(no) * min(yes)))), largest_without_gain=max(no), smallest_with_gain=min(yes))
    else:
        gate = dict(gate_subblocks=None, note="the measured sizes do not split into no gain below, gain above", without_gain=no, with_gain=yes)
    lines.append(gate)
    print(json.dumps(gate), flush=True)
    with open(os.path.join(a.out_dir, "x_tile_drop_by_size.jsonl"), "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
