#!/usr/bin/env python3
"""The stop test of the one-polynomial block loop (dkmc_set_x_stop_form; DESIGN.md sections 6 and 9) in the headline's own regime.

  python tools/x_stop_bench.py run FORM KAPPA RECORD_FILE [bench.py arguments ...]
      one bench.py run with dkmc_set_x_stop_form(FORM) and dkmc_set_x_stop_margin(KAPPA) (FORM = default: the library's switches untouched); the result
      line goes to stdout as bench.py prints it, one JSON record is appended to RECORD_FILE: steps/s, sweeps per step, and of every timed step which test
      ended the loop (1 bound, 2 norm), ||Rt(:, 0)|| and (Rt'Z)_00 at the stop, the true residual, re-entry rounds (dkmc_stats.x_tile_f64_rounds).
  python tools/x_stop_bench.py soak WORKLOAD STEPS RECORD_FILE KAPPA [KAPPA ...]
      STEPS coupled supersteps (after 2 untimed ones) under form 1 at each margin, one process each under its own time limit (the pattern of
      tools/soak_tile_drop.py), after one under form 0; per process a record: sweeps per step, steps with a re-entry round, the largest true residual over
      tol, steps the norm test ended, a hash of the event logs; then the verdict: the largest margin without a re-entry round.
"""
import contextlib
import ctypes as C
import hashlib
import io
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stop_info(L):
    f = C.c_int(-1); a = [C.c_double(), C.c_double(), C.c_double()]
    L.dkmc_get_x_stop_info(C.byref(f), C.byref(a[0]), C.byref(a[1]), C.byref(a[2]))
    return f.value, a[0].value, a[1].value, a[2].value


def switches(L, form, kappa):
    if form != "default":
        L.dkmc_set_x_stop_form(int(form)); L.dkmc_set_x_stop_margin(float(kappa))


class Tee(io.StringIO):
    def write(self, s):
        sys.__stdout__.write(s)
        return super().write(s)


def run(form, kappa, record, argv):
    import bench
    from devicekmc_amd import host, lib
    L = lib.load()
    switches(L, form, kappa)
    solves = []
    step0 = bench.Sim.step

    def step(self, timed):
        t = step0(self, timed)
        if timed:
            st = host.get_stats()
            solves.append(stop_info(L) + (int(st["x_tile_f64_rounds"]), int(st["cg_iters_X"])))
        return t
    bench.Sim.step = step
    sys.argv = [os.path.join(ROOT, "bench.py")] + argv
    buf = Tee()
    with contextlib.redirect_stdout(buf):
        bench.main()
    line = json.loads([x for x in buf.getvalue().splitlines() if x.startswith("{")][-1])
    tol = line["config"]["cg_tol"]
    rec = {"workload": line["config"]["workload"], "rows": line["config"]["atoms"] + 1, "stop_form": L.dkmc_get_x_stop_form(), "kappa": L.dkmc_get_x_stop_margin(),
           "steps": line["steps"], "warmup": line["warmup"], "steps_per_s": line["value"], "ms_per_step": line["ms_per_step"],
           "sweeps_per_step": line["per_step"]["cg_iters_X"], "sweeps_each": [s[5] for s in solves[:64]], "fired_each": [s[0] for s in solves[:64]],
           "norm_at_stop_each": [float("%.3e" % s[1]) for s in solves[:64]], "rz_at_stop_each": [float("%.3e" % s[2]) for s in solves[:64]],
           "true_residual_each": [float("%.3e" % s[3]) for s in solves[:64]], "true_residual_max_over_tol": max(s[3] for s in solves) / tol,
           "steps_ended_by_the_norm": sum(1 for s in solves if s[0] == 2), "reentered_steps": sum(1 for s in solves if s[4] > 0), "cg_tol": tol}
    with open(record, "a") as f:
        f.write(json.dumps(rec) + "\n")


def soak_child(name, form, kappa, steps, path):
    import numpy as np
    import torch
    from bench import Sim
    from devicekmc_amd import host, lib
    L = lib.load()
    switches(L, form, kappa)
    sim = Sim(name, "cuda:0")
    for _ in range(2):
        sim.step(False)
    tol = sim.p.cg_tol
    sweeps, fired, rounds, res, h, ims = [], [], 0, 0.0, hashlib.sha1(), []
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
        sweeps.append(int(st["cg_iters_X"])); fired.append(stop_info(L)[0]); rounds += st["x_tile_f64_rounds"] > 0
        res = max(res, math.sqrt(max(st["cg_rr_X"], 0.0)))
        h.update(np.ascontiguousarray(np.array(sim.kmc.last_event_log)).tobytes()); h.update(np.float64(dt).tobytes()); ims.append(float(dev.imacro))
    el = time.perf_counter() - t0
    with open(path, "w") as f:
        f.write(json.dumps(dict(workload=name, stop_form=L.dkmc_get_x_stop_form(), kappa=L.dkmc_get_x_stop_margin(), steps=steps, steps_per_s=round(steps / el, 4),
                                sweeps_per_step=sum(sweeps) / steps, sweeps_each=sweeps, steps_ended_by_the_norm=sum(1 for x in fired if x == 2),
                                steps_with_reentry=int(rounds), true_residual_max_over_tol=res / tol, events_sha1=h.hexdigest()[:16], I_macro_each=ims)) + "\n")
    sim.close()


def soak(name, steps, record, kappas, limit=300):
    recs = []
    for form, kappa in [("0", 1.0)] + [("1", k) for k in kappas]:
        part = record + ".part"
        try:
            rc = subprocess.call([sys.executable, os.path.abspath(__file__), "soak-child", name, form, repr(kappa), str(steps), part], timeout=limit)
        except subprocess.TimeoutExpired:
            rc = 124
        if rc:
            print("form %s kappa %s: process ended with %d" % (form, kappa, rc), file=sys.stderr)
            sys.exit(1)                   # nothing more is started on the GPU after a failure
        recs.append(json.loads(open(part).read())); os.remove(part)
    base = recs[0]
    for r in recs[1:]:
        r["same_events_as_form_0"] = r["events_sha1"] == base["events_sha1"]
        r["rel_dI_macro_max"] = max(abs(b / a - 1) for a, b in zip(base["I_macro_each"], r["I_macro_each"]))
    ok = [r["kappa"] for r in recs[1:] if r["steps_with_reentry"] == 0 and r["true_residual_max_over_tol"] <= 1.0]
    verdict = dict(verdict="largest margin without a re-entry round", workload=name, steps=steps, kappa=max(ok) if ok else None,
                   sweeps_per_step={("form 0" if r["stop_form"] == 0 else "kappa %.4f" % r["kappa"]): r["sweeps_per_step"] for r in recs})
    with open(record, "a") as f:
        for r in recs:
            r.pop("I_macro_each")
            f.write(json.dumps(r) + "\n")
        f.write(json.dumps(verdict) + "\n")
    print(json.dumps(verdict))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5:])
    elif sys.argv[1] == "soak":
        soak(sys.argv[2], int(sys.argv[3]), sys.argv[4], [float(x) for x in sys.argv[5:]])
    elif sys.argv[1] == "soak-child":
        soak_child(sys.argv[2], sys.argv[3], float(sys.argv[4]), int(sys.argv[5]), sys.argv[6])
