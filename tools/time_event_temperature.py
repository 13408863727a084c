#!/usr/bin/env python3
"""What the event rates on the local site temperature (dkmc_set_event_temperature) and the rate census (dkmc_set_event_census) cost.  One child
process per workload; a workload name may end in ":nocurrent" (the current solve off).  In it the cases mode 0, 1, 0, 2, 0 and mode 0 with the
census on, in that order: one untimed superstep, then `steps` timed ones, with the HIP-event time of k_ev_build and of the census of every timed step
(dkmc_debug_get_event_times under dkmc_set_profiling(1)) and the supersteps per second over the timed steps.  site_temperature is the uniform
field the host initialises it with (the workloads run without the local heat model): the cost of the build does not depend on the values, and the
cases continue one trajectory.  A difference counts only above 3 x the spread
of the three mode-0 cases of the same process.  The census is also set against its algorithmic bytes (12 B per slot + 4 B per live slot).
One JSON line per workload in <out-dir>/event_temperature_by_size.jsonl.
usage: python tools/time_event_temperature.py [7.5nm tile:10 tile:20:nocurrent] [--steps 5] [--out-dir profiles]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT_NAME = "event_temperature_by_size.jsonl"
CASES = [("mode0_a", 0, False), ("mode1", 1, False), ("mode0_b", 0, False), ("mode2", 2, False), ("mode0_c", 0, False), ("mode0_census", 0, True)]


def child(spec, steps, out_dir):
    import torch
    from bench import Sim
    from devicekmc_amd import lib
    L = lib.load()
    nocurrent = spec.endswith(":nocurrent")
    name = spec[:-len(":nocurrent")] if nocurrent else spec
    sim = Sim(name, "cuda:0", solve_current=False if nocurrent else None)
    ms2 = (C.c_double * 2)()
    cases = {}
    L.dkmc_set_profiling(1)
    try:
        for label, mode, census in CASES:
            sim.p.event_temperature, sim.p.event_census = mode, census
            sim.step(False)
            build, cen, live = [], [], 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                sim.step(True)
                lib.check(L.dkmc_debug_get_event_times(ms2))
                build.append(ms2[0]); cen.append(ms2[1])
                if census:
                    live = sim.kmc.last_event_census["n_live"]
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            cases[label] = dict(mode=mode, census=census, build_ms=round(statistics.median(build), 6), build_ms_min=round(min(build), 6),
                                build_ms_max=round(max(build), 6), census_ms=round(statistics.median(cen), 6), steps_per_s=round(steps / el, 4),
                                live_slots=live)
    finally:
        L.dkmc_set_profiling(0)
        sim.p.event_temperature, sim.p.event_census = 0, False
    N, nn = int(sim.dev.N), int(sim.gb.nn_)
    base = [cases[k] for k in ("mode0_a", "mode0_b", "mode0_c")]
    rec = dict(workload=spec, sites=N, nn=nn, slots=N * nn, steps=steps, cases=cases)
    for key in ("build_ms", "steps_per_s"):
        v = [c[key] for c in base]
        mean, spr = sum(v) / 3, max(v) - min(v)
        rec[key + "_mode0_mean"], rec[key + "_mode0_spread"] = round(mean, 6), round(spr, 6)
        for label in ("mode1", "mode2", "mode0_census"):
            d = cases[label][key] - mean
            rec["%s_%s_diff" % (key, label)] = round(d, 6)
            rec["%s_%s_counts" % (key, label)] = bool(abs(d) > 3 * spr)
    c = cases["mode0_census"]
    census_bytes = 12 * N * nn + 4 * c["live_slots"]
    rec["census_bytes"] = census_bytes
    rec["census_GBs"] = round(census_bytes / (c["census_ms"] * 1e-3) / 1e9, 2) if c["census_ms"] > 0 else None
    rec["census_share_of_step"] = round(c["census_ms"] * 1e-3 * c["steps_per_s"], 6)
    sim.close()
    line = json.dumps(rec)
    with open(os.path.join(out_dir, OUT_NAME), "a") as f:
        f.write(line + "\n")
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=["7.5nm", "tile:10", "tile:20:nocurrent"])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--append", action="store_true", help="keep the records already in the output file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.steps, a.out_dir)
    os.makedirs(a.out_dir, exist_ok=True)
    if not a.append:
        open(os.path.join(a.out_dir, OUT_NAME), "w").close()
    bad = 0
    for name in a.workloads:      # one process per workload: every workload starts from a fresh library and allocator
        rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--child", name, "--steps", str(a.steps), "--out-dir", a.out_dir])
        if rc:
            print("%s: child ended with %d" % (name, rc), file=sys.stderr)
            bad = 1
            break                 # nothing more is started on the GPU after a failure
    sys.exit(bad)


if __name__ == "__main__":
    main()
