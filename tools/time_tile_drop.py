#!/usr/bin/env python3
"""Sweeps on the live tiles only (dkmc_set_x_tile_drop) against the full image, on whole supersteps.  One child process per workload; in it the cases
theta = 0, 1e-12, 0, 1e-11, 0, 1e-10, 0, 1e-9 run one after the other, each on a fresh device with the same seeds: `warmup` untimed supersteps, then
`steps` timed ones with profiling on.  The four theta = 0 cases are the reference point and give its run-to-run spread (the project's rule: a
difference counts when it exceeds 3 x that spread).  Per case one JSON line in <out-dir>/x_tile_drop_<workload>.jsonl: supersteps/s, sweeps per
step, dkmc_stats.x_tile_f64_rounds summed over the timed steps, the largest true residual of a timed solve, the eight words of
dkmc_get_x_tile_live_info of the last step (state, tiles stored / live, sub-blocks stored / in live tiles / live on their own, bytes of the compact
image, sweeps on it), ms2 averaged over the timed steps (census + scan, compaction + view build), the largest relative difference of I_macro and of
site_power against the FIRST theta = 0 case of the same process over all timed steps, and whether the event logs are equal to that case's.
--units 0 1 (dkmc_set_x_tile_drop_unit: whole tiles against sub-blocks): the cases are theta = 0, (1e-10, unit 0), 0, (1e-10, unit 1), 0, (1e-12, unit 0),
0, (1e-12, unit 1) instead, every record carries its unit, and the file is <out-dir>/x_tile_drop_unit_<workload>.jsonl.  The default, unit 0 alone,
gives the cases, records and file described first.
usage: python tools/time_tile_drop.py [7.5nm tile:5 tile:10] [--steps 6] [--warmup 2] [--units 0 1] [--out-dir profiles]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (0.0, 1e-12, 0.0, 1e-11, 0.0, 1e-10, 0.0, 1e-9)
UNIT_THETAS = (1e-10, 1e-12)


def cases(units):
    """(theta, unit or None) in running order; None: the unit is not part of the record (the default: unit 0 alone)"""
    if list(units) == [0]:
        return [(theta, None) for theta in CASES]
    return [c for theta in UNIT_THETAS for u in units for c in ((0.0, 0), (theta, u))]


def run(name, theta, steps, warmup, unit=None):
    import numpy as np
    import torch
    from bench import Sim
    from devicekmc_amd import host, lib
    L = lib.load()
    L.dkmc_set_x_tile_drop(theta); L.dkmc_set_x_tile_drop_unit(unit or 0)
    L.dkmc_set_x_tile_drop_auto(0)                    # the cases are explicit thresholds: theta = 0 is the full view at every size
    try:
        sim = Sim(name, "cuda:0")
        for _ in range(warmup):
            sim.step(False)
        L.dkmc_set_profiling(1)
        info, ms = (C.c_longlong * 8)(), (C.c_double * 2)()
        sweeps = rounds = 0; rr = 0.0; ms2 = [0.0, 0.0]; im = []; power = []; logs = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            dev, gb, p = sim.dev, sim.gb, sim.p
            dev.updateCharge(gb); dev.updatePotential(gb, p, sim.Vd, sim.k)
            _, dt = sim.kmc.executeKMCStep(gb, dev, want_log=True)
            dev.updatePower(gb, p, sim.Vd); dev.updateTemperature(gb, p, dt)
            torch.cuda.synchronize()
            sim.k += 1
            st = host.get_stats()
            ms[0] = ms[1] = 0.0
            lib.check(L.dkmc_get_x_tile_live_info(info, ms))
            sweeps += st["cg_iters_X"]; rounds += st["x_tile_f64_rounds"]; rr = max(rr, st["cg_rr_X"]); ms2[0] += ms[0]; ms2[1] += ms[1]
            im.append(dev.imacro); power.append(gb.site_power.cpu().numpy().copy()); logs.append(np.array(sim.kmc.last_event_log).copy())
        el = time.perf_counter() - t0
        rec = dict(workload=name, theta=theta, sites=int(sim.s.N), steps=steps, steps_per_s=round(steps / el, 4), sweeps_per_step=round(sweeps / steps, 2),
                   x_tile_f64_rounds=int(rounds), true_residual=float(np.sqrt(rr)), info8=[int(v) for v in info],
                   ms2=[round(ms2[0] / steps, 4), round(ms2[1] / steps, 4)])
        if unit is not None:
            rec["unit"] = unit
        sim.close()
        return rec, (im, power, logs)
    finally:
        L.dkmc_set_x_tile_drop(0.0); L.dkmc_set_x_tile_drop_unit(0); L.dkmc_set_x_tile_drop_auto(1); L.dkmc_set_profiling(0)


def child(name, steps, warmup, out_dir, units):
    import numpy as np
    path = os.path.join(out_dir, "x_tile_drop_%s%s.jsonl" % ("" if list(units) == [0] else "unit_", name.replace(":", "")))
    ref = None
    with open(path, "w") as f:
        for theta, unit in cases(units):
            rec, got = run(name, theta, steps, warmup, unit)
            if ref is None:
                ref = got
            rec["rel_dI_macro"] = float(max(abs(a / b - 1) for a, b in zip(got[0], ref[0])))
            rec["rel_dsite_power"] = float(max(np.abs(a - b).max() / np.abs(b).max() for a, b in zip(got[1], ref[1])))
            rec["event_logs_equal"] = bool(all(np.array_equal(a, b) for a, b in zip(got[2], ref[2])))
            line = json.dumps(rec)
            f.write(line + "\n"); f.flush()
            print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=["7.5nm", "tile:5", "tile:10"])
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--units", type=int, nargs="+", choices=[0, 1], default=[0], help="dkmc_set_x_tile_drop_unit of the cases (default: 0 alone, the cases of CASES)")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.steps, a.warmup, a.out_dir, a.units)
    os.makedirs(a.out_dir, exist_ok=True)
    bad = 0
    for name in a.workloads:      # one process per workload: every workload starts from a fresh library and allocator
        rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--child", name, "--steps", str(a.steps), "--warmup", str(a.warmup), "--out-dir", a.out_dir,
                              "--units"] + [str(u) for u in a.units])
        if rc:
            print("%s: child ended with %d" % (name, rc), file=sys.stderr)
            bad = 1
            break                 # nothing more is started on the GPU after a failure
    sys.exit(bad)


if __name__ == "__main__":
    main()
