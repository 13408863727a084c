#!/usr/bin/env python3
"""The local heat model on the general CSR loop (dkmc_set_heat_form(0), the reference point) against the pattern-only CG of the K solve
(dkmc_set_heat_form(1)) with every sub-step polled (dkmc_debug_heat_chain(0, 0)) and with the sub-steps chained on the device (the default), in one
process on one GPU.  Per mode one transient update of `n` sub-steps from the background temperature and one steady update, both timed from the call
to the synchronised return after one untimed update of each kind; the power is a synthetic smooth field scaled so that a sub-step heats by at most
30 K (the current solve is off).  Prints one JSON line per mode: ms per sub-step, iterations, host synchronisations, form.
usage: python tools/time_heat_forms.py [7.5nm tile:10 ...] [--substeps 100] [--large 0|1]   (--large 1: dkmc_set_k_blocked_large, the windowed form above 262 144 rows)"""
import argparse
import ctypes as C
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T_1 = 50.0


def smooth_power(dev, p):
    import numpy as np
    lo, m = dev.N_left_tot, dev.N_interface
    x, y, z = (np.asarray(a, dtype=np.float64) for a in (dev.site_x, dev.site_y, dev.site_z))
    f = (1.5 + np.cos(2 * np.pi * y / (np.ptp(y) + 1.0)) * np.cos(2 * np.pi * z / (np.ptp(z) + 1.0))) * np.exp(-((x - x.mean()) / (0.25 * np.ptp(x) + 1.0)) ** 2)
    P = np.zeros(dev.N)
    P[lo:lo + m] = f[lo:lo + m]
    c = 1.0 / ((p.nn_dist * 1e-10 * min(p.k_th_interface, p.k_th_vacancies)) * abs(T_1 - p.background_temp))
    return P * 30.0 / (P.max() * c * p.delta_t * p.tau * abs(T_1 - p.background_temp))


def run(name, mode, n, large):
    import numpy as np
    import torch
    from bench import make_workload
    from devicekmc_amd import host, lib
    L = lib.load()
    form, chain = {"switch0": (0, 1), "switch1_polled": (1, 0), "switch1_chained": (1, 1)}[mode]
    L.dkmc_set_heat_form(form); L.dkmc_debug_heat_chain(chain, 0); L.dkmc_set_k_blocked_large(large)
    try:
        s, p = make_workload(name)
        p.solve_current = False; p.solve_heating_global = False; p.solve_heating_local = True
        dev = host.Device(s, p, gpu_neighbors="cuda:0")
        gb = dev.make_gpubuf("cuda:0")
        dev.constructLaplacian(gb, p)
        gb.site_power.copy_(torch.as_tensor(smooth_power(dev, p)))
        out = dict(workload=name, sites=int(s.N), rows=int(dev.N_interface), mode=mode, k_blocked_large=large)
        for kind, step_time in (("transient", (n - 0.5) * p.delta_t), ("steady", 2e3 * p.delta_t)):
            for timed in (0, 1):
                gb.site_temperature.fill_(p.background_temp)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dev.updateTemperature(gb, p, step_time)
                torch.cuda.synchronize()
                ms = 1e3 * (time.perf_counter() - t0)
            info = dev.last_heat_info
            sub = dev.last_heat_solves
            out[kind] = dict(sub_steps=sub, ms=round(ms, 3), ms_per_sub_step=round(ms / sub, 4), iterations=dev.last_heat_cg_iters,
                             host_syncs=info["host_syncs"], resumed=info["resumed_sub_steps"], form=info["form"], bytes_per_iteration=info["bytes_per_iteration"],
                             max_rise_K=round(float((gb.site_temperature - p.background_temp).abs().max().item()), 3))
        del dev, gb
        torch.cuda.empty_cache()
        return out
    finally:
        L.dkmc_set_heat_form(0); L.dkmc_debug_heat_chain(1, 0); L.dkmc_set_k_blocked_large(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=["7.5nm"])
    ap.add_argument("--substeps", type=int, default=100)
    ap.add_argument("--large", type=int, default=0)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    for name in a.workloads:
        for mode in ("switch0", "switch1_polled", "switch1_chained"):
            print(json.dumps(run(name, mode, a.substeps, a.large)), flush=True)


if __name__ == "__main__":
    main()
