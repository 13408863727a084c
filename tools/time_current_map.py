#!/usr/bin/env python3
"""What the current map (dkmc_set_current_map) costs per current solve.  One child process per workload.  In it: `warmup` untimed supersteps and
`steps` timed ones with the switch off (the build's own step time), then the fields of one more step up to the KMC events, and on THAT state
`repeats` + 1 rounds of Device.updatePower with the switch 0 and then 1 -- before every call the start vector of the solve (the private warm-start
copy and atom_virtual_potentials) is put back, so that all calls run the same solve; the first round is discarded.  With the switch on the call
also copies the three site arrays and the summary to the host (Device._fetch_current_map); that copy is timed once more on its own after each
switch-1 call, so that the record separates the device work (tile passes + row kernel + fold) from the copy.
One JSON line per workload in <out-dir>/current_map_7p5_tile10.jsonl: median and spread (min, max) of the call with the switch off and on, of the
copy, the difference of the medians with and without the copy, the CG sweeps of the calls (equal: the switch does not touch the solve), the summary
of the map, and the step time with the switch off.
usage: python tools/time_current_map.py [7.5nm tile:10] [--repeats 5] [--steps 3] [--warmup 2] [--out-dir profiles]"""
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

OUT_NAME = "current_map_7p5_tile10.jsonl"


def spread(v):
    return dict(median=round(statistics.median(v), 6), min=round(min(v), 6), max=round(max(v), 6), n=len(v))


def child(name, repeats, steps, warmup, out_dir):
    import numpy as np
    import torch
    from bench import Sim
    from devicekmc_amd import host, lib
    L = lib.load()
    L.dkmc_set_current_map(0)
    sim = Sim(name, "cuda:0")
    for _ in range(warmup):
        sim.step(False)
    step_s = [sim.step(True) for _ in range(steps)]
    dev, gb, p, V = sim.dev, sim.gb, sim.p, sim.Vd
    dev.updateCharge(gb); dev.updatePotential(gb, p, V, sim.k)
    sim.kmc.executeKMCStep(gb, dev)
    n = C.c_int(0)
    lib.check(L.dkmc_get_current_warm_vector(C.byref(gb.c), None, 0, C.byref(n)))
    warm = np.zeros(n.value)
    lib.check(L.dkmc_get_current_warm_vector(C.byref(gb.c), warm.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
    m0 = gb.atom_virtual_potentials.clone()
    t = {0: [], 1: []}; fetch = []; sweeps = {0: [], 1: []}
    try:
        for r in range(repeats + 1):
            for sw in (0, 1):
                lib.check(L.dkmc_set_current_warm_vector(C.byref(gb.c), warm.ctypes.data_as(C.c_void_p), len(warm)))
                gb.atom_virtual_potentials.copy_(m0)
                L.dkmc_set_current_map(sw)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dev.updatePower(gb, p, V)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                if sw:
                    dev._fetch_current_map(gb)
                    t2 = time.perf_counter()
                if r > 0:
                    t[sw].append(t1 - t0); sweeps[sw].append(int(host.get_stats()["cg_iters_X"]))
                    if sw:
                        fetch.append(t2 - t1)
    finally:
        L.dkmc_set_current_map(0)
    info = dict(dev.current_map_info)
    st = host.get_stats()
    d = statistics.median(t[1]) - statistics.median(t[0])
    rec = dict(workload=name, sites=int(sim.s.N), rows=int(info["rows"]), xt_ns=int(st["xt_ns"]), tile_store_bytes=int(st["xt_subblocks"]) * 8192,
               tile_passes=int(info["tile_passes"]), power_off_s=spread(t[0]), power_on_s=spread(t[1]), host_copy_s=spread(fetch),
               map_cost_ms=round(1e3 * d, 3), map_device_ms=round(1e3 * (d - statistics.median(fetch)), 3),
               sweeps_off=sweeps[0], sweeps_on=sweeps[1], step_off_s=spread(step_s),
               I_macro=info["I_macro"], I_driver0=info["I_driver0"], max_node_defect=info["max_node_defect"],
               sum_current=info["sum_current"], sum_current_tunnel=info["sum_current_tunnel"])
    sim.close()
    line = json.dumps(rec)
    with open(os.path.join(out_dir, OUT_NAME), "a") as f:
        f.write(line + "\n")
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=["7.5nm", "tile:10"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.repeats, a.steps, a.warmup, a.out_dir)
    os.makedirs(a.out_dir, exist_ok=True)
    open(os.path.join(a.out_dir, OUT_NAME), "w").close()
    bad = 0
    for name in a.workloads:      # one process per workload: every workload starts from a fresh library and allocator
        rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--child", name, "--repeats", str(a.repeats), "--steps", str(a.steps),
                              "--warmup", str(a.warmup), "--out-dir", a.out_dir])
        if rc:
            print("%s: child ended with %d" % (name, rc), file=sys.stderr)
            bad = 1
            break                 # nothing more is started on the GPU after a failure
    sys.exit(bad)


if __name__ == "__main__":
    main()
