#!/usr/bin/env python3
"""The two forms of the pair sum's kernels (dkmc_set_pair_form: 0 evaluates a term where it is tested, 1 queues the passing pairs per wave and
evaluates 64 at a time) on the same workloads with the current solve off.  Per workload the cases 0, 1, 0, 1, 0 run in one process, each on a fresh
device: one untimed superstep, then `steps` supersteps (charge + potential + events) with profiling on.  The three form-0 cases give the run-to-run
spread of the reference point.  Per case one JSON line: sites, charged sites of the last step, the kernel that summed, pairs tested / evaluated,
the lane slots of the expensive part (dkmc_get_pair_sum_info: what form 0 spends, what form 1 issued; counted by form 1 only), the mean HIP-event
time per call of the sum kernels alone and of the whole call, supersteps/s, and a sha256 of site_potential_charge after the last step -- which must
be the same in all five cases.
usage: python tools/time_pair_forms.py [tile:20 tile:10 7.5nm] [--steps 5]"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Vd = 5.0


def run(name, form, steps):
    import torch
    from bench import make_workload
    from devicekmc_amd import host, lib
    L = lib.load()
    L.dkmc_set_pair_form(form)
    try:
        s, p = make_workload(name)
        p.solve_current = False; p.solve_heating_global = False
        dev = host.Device(s, p, gpu_neighbors="cuda:0")
        sim = host.KMCProcess(dev, p.freq)
        gb = dev.make_gpubuf("cuda:0")
        dev.setLaplacePotential(gb, p, Vd)
        gb.sync_HostToGPU(dev)
        dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, 0)
        sim.executeKMCStep(gb, dev)
        L.dkmc_set_profiling(1)
        info, ms = (C.c_longlong * 6)(), (C.c_double * 2)()
        sum_ms = call_ms = 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(1, steps + 1):
            dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, k)
            lib.check(L.dkmc_get_pair_sum_info(info, ms))
            call_ms += ms[0]; sum_ms += ms[1]
            if k == steps:                  # the record is of the last pair sum: copy its potentials before the events change the device
                pc = gb.site_potential_charge.cpu().numpy().copy()
                charged = int((gb.site_charge != 0).sum().item())
                st = host.get_stats()
            sim.executeKMCStep(gb, dev)
        torch.cuda.synchronize()
        rate = steps / (time.perf_counter() - t0)
        out = dict(workload=name, form=int(info[0]), sites=int(s.N), charged=charged, kernel="k_pairwise_cells" if info[1] else "k_pairwise",
                   workgroups=int(info[2]), pairs_tested=int(st["pair_tested"]), pairs_evaluated=int(st["pair_evaluated"]),
                   slots_form0=int(info[3]), slots_form1=int(info[4]),
                   evaluated_per_slot_form1=round(st["pair_evaluated"] / info[4], 4) if info[4] > 0 else None,
                   slots_form0_over_form1=round(info[3] / info[4], 3) if info[4] > 0 else None,
                   sum_kernel_ms=round(sum_ms / steps, 4), pair_call_ms=round(call_ms / steps, 4), steps_per_s=round(rate, 3),
                   sha256_potential_charge=hashlib.sha256(pc.tobytes()).hexdigest())
        del gb, sim, dev
        torch.cuda.empty_cache()
        return out
    finally:
        L.dkmc_set_pair_form(0); L.dkmc_set_profiling(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=["tile:20", "tile:10", "7.5nm"])
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    bad = 0
    for name in a.workloads:
        hashes = set()
        for form in (0, 1, 0, 1, 0):
            rec = run(name, form, a.steps)
            hashes.add(rec["sha256_potential_charge"])
            print(json.dumps(rec), flush=True)
        if len(hashes) != 1:
            print("%s: the potentials of the five cases differ" % name, file=sys.stderr)
            bad = 1
    sys.exit(bad)


if __name__ == "__main__":
    main()
