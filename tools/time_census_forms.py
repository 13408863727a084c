#!/usr/bin/env python3
"""The census of the live view on the fp64 store (form 0) against the census on the fp32 image with its guard band (form 1;
dkmc_debug_xtl_census_form, csrc/xt_live.h), per solve, inside coupled supersteps of one process: after `warmup` untimed steps the forms alternate step
by step, with profiling on, and every step records ms2[0] of dkmc_get_x_tile_live_info (census + the two scans), ms2[1] (compaction + view build),
the report's counts and the sub-blocks the image form read again from the fp64 store.  The closing line: the medians, form 0's spread
(max - min) / median, and `adopt` -- form 1's median is below form 0's by more than 3 x that spread (the project's rule).
usage: python tools/time_census_forms.py [tile:10] [--solves 6] [--warmup 2] [--out profiles/x_tile_census_forms_tile10.jsonl]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="tile:10")
    ap.add_argument("--solves", type=int, default=6, help="solves per form")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "x_tile_census_forms_tile10.jsonl"))
    a = ap.parse_args()
    import torch
    from bench import Sim
    from devicekmc_amd import lib
    L = lib.load()
    L.dkmc_set_x_tile_drop(1e-10)
    was = L.dkmc_debug_xtl_census_form(0)
    recs = []
    try:
        sim = Sim(a.workload, "cuda:0")
        for _ in range(a.warmup):
            sim.step(False)
        L.dkmc_set_profiling(1)
        info, ms = (C.c_longlong * 8)(), (C.c_double * 2)()
        for k in range(2 * a.solves):
            form = k & 1
            L.dkmc_debug_xtl_census_form(form)
            sim.step(False)
            torch.cuda.synchronize()
            ms[0] = ms[1] = 0.0
            lib.check(L.dkmc_get_x_tile_live_info(info, ms))
            recs.append(dict(workload=a.workload, step=k, form=form, census_ms=round(ms[0], 4), compact_ms=round(ms[1], 4), info8=[int(v) for v in info],
                             reread_subblocks=int(L.dkmc_debug_xtl_census_reread())))
            print(json.dumps(recs[-1]), flush=True)
        sim.close()
    finally:
        L.dkmc_set_profiling(0); L.dkmc_set_x_tile_drop(0.0); L.dkmc_debug_xtl_census_form(was)
    t0 = [r["census_ms"] for r in recs if r["form"] == 0]; t1 = [r["census_ms"] for r in recs if r["form"] == 1]
    m0, m1 = statistics.median(t0), statistics.median(t1)
    spread = (max(t0) - min(t0)) / m0
    verdict = dict(workload=a.workload, solves_per_form=a.solves, census_ms_form0_median=m0, census_ms_form1_median=m1, spread_form0=round(spread, 5),
                   ratio=round(m1 / m0, 4), adopt=bool(m1 < m0 * (1.0 - 3.0 * spread)))
    print(json.dumps(verdict))
    with open(a.out, "w") as f:
        for r in recs + [verdict]:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
