#!/usr/bin/env python3
"""The longer run behind the live view's auto mode (dkmc_set_x_tile_drop_auto): coupled supersteps of one workload with auto mode off and with auto mode
on, same seeds, one process each under its own time limit.  After `warmup` untimed supersteps every step is recorded: sweeps,
dkmc_stats.x_tile_f64_rounds (re-entry rounds on the fp64 store), the true residual of column 0, dkmc_get_x_tile_drop_used(), live tiles and sub-blocks
in them, dt, I_macro and a hash of the event log.  A closing line per process (steps/s, steps with a re-entry round, the largest true residual) and one
for the pair: event logs identical, every true residual within tol^2, steps with a re-entry round, largest relative difference of I_macro.

--theta T runs the second process with auto mode off and the explicit threshold T instead (the fallback thresholds 1e-11 and 1e-12).
usage: python tools/soak_tile_drop.py [tile:10] [--steps 100] [--warmup 2] [--limit 300] [--theta 0] [--out profiles/x_tile_drop_soak_tile10.jsonl]"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(name, mode, theta, steps, warmup, path):
    import numpy as np
    import torch
    from bench import Sim
    from devicekmc_amd import host, lib
    L = lib.load()
    L.dkmc_set_x_tile_drop_auto(1 if mode == "auto_on" else 0)
    L.dkmc_set_x_tile_drop(theta if mode == "explicit" else 0.0)
    sim = Sim(name, "cuda:0")
    for _ in range(warmup):
        sim.step(False)
    info, ms = (C.c_longlong * 8)(), (C.c_double * 2)()
    tol2 = sim.p.cg_tol ** 2
    rounds_steps = 0; rr_max = 0.0
    with open(path, "w") as f:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(steps):
            dev, gb, p = sim.dev, sim.gb, sim.p
            dev.updateCharge(gb); dev.updatePotential(gb, p, sim.Vd, sim.k)
            _, dt = sim.kmc.executeKMCStep(gb, dev, want_log=True)
            dev.updatePower(gb, p, sim.Vd); dev.updateTemperature(gb, p, dt)
            torch.cuda.synchronize()
            sim.k += 1
            st = host.get_stats()
            lib.check(L.dkmc_get_x_tile_live_info(info, ms))
            log = np.ascontiguousarray(np.array(sim.kmc.last_event_log))
            rec = dict(mode=mode, step=k, sweeps=int(st["cg_iters_X"]), x_tile_f64_rounds=int(st["x_tile_f64_rounds"]), true_residual=float(np.sqrt(max(st["cg_rr_X"], 0.0))),
                       within_tol=bool(st["cg_rr_X"] <= tol2), used=L.dkmc_get_x_tile_drop_used(), live_tiles=int(info[2]), live_subblocks=int(info[4]),
                       stored_subblocks=int(st["xt_subblocks"]), dt=float(dt), I_macro=float(dev.imacro), event_log_sha1=hashlib.sha1(log.tobytes()).hexdigest()[:16])
            rounds_steps += rec["x_tile_f64_rounds"] > 0; rr_max = max(rr_max, rec["true_residual"])
            f.write(json.dumps(rec) + "\n")
        el = time.perf_counter() - t0
        f.write(json.dumps(dict(mode=mode, workload=name, sites=int(sim.s.N), steps=steps, warmup=warmup, theta=theta if mode == "explicit" else None,
                                steps_per_s=round(steps / el, 4), steps_with_reentry=int(rounds_steps), true_residual_max=rr_max, cg_tol=float(sim.p.cg_tol))) + "\n")
    sim.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="tile:10")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=300, help="time limit of one process, seconds")
    ap.add_argument("--theta", type=float, default=0.0, help="> 0: the second process runs this explicit threshold with auto mode off")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "x_tile_drop_soak_tile10.jsonl"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.workload, a.child, a.theta, a.steps, a.warmup, a.out)
    runs = {}
    for mode in ("auto_off", "explicit" if a.theta > 0 else "auto_on"):
        part = a.out + "." + mode
        try:
            rc = subprocess.call([sys.executable, os.path.abspath(__file__), a.workload, "--child", mode, "--theta", str(a.theta), "--steps", str(a.steps),
                                  "--warmup", str(a.warmup), "--out", part], timeout=a.limit)
        except subprocess.TimeoutExpired:
            rc = 124
        if rc:
            print("%s: process ended with %d" % (mode, rc), file=sys.stderr)
            sys.exit(1)               # nothing more is started on the GPU after a failure
        runs[mode] = [json.loads(x) for x in open(part)]
        os.remove(part)
    (ma, a_), (mb, b_) = runs.items()
    sa, sb = a_[:-1], b_[:-1]
    verdict = dict(pair=[ma, mb], steps=len(sa), event_logs_identical=bool(all(x["event_log_sha1"] == y["event_log_sha1"] and x["dt"] == y["dt"] for x, y in zip(sa, sb))),
                   every_true_residual_within_tol=bool(all(x["within_tol"] for x in sa + sb)), steps_with_reentry={ma: a_[-1]["steps_with_reentry"], mb: b_[-1]["steps_with_reentry"]},
                   steps_on_the_live_view=sum(1 for y in sb if y["used"] > 0), rel_dI_macro_max=max(abs(y["I_macro"] / x["I_macro"] - 1) for x, y in zip(sa, sb)),
                   steps_per_s={ma: a_[-1]["steps_per_s"], mb: b_[-1]["steps_per_s"]})
    with open(a.out, "w") as f:
        for rec in a_ + b_ + [verdict]:
            f.write(json.dumps(rec) + "\n")
    print(json.dumps(a_[-1])); print(json.dumps(b_[-1])); print(json.dumps(verdict))


if __name__ == "__main__":
    main()
