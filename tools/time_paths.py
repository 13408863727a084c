#!/usr/bin/env python3
"""What the conduction-path analysis (dkmc_find_paths) costs, against the two things it is measured by.  One child process per workload.  In it:
a simulation with the current solve off, `warmup` untimed and `steps` timed supersteps (the step the analysis would gate); then, on the pristine
device and on the same device with a planted bridging filament (every O site within 3 A of the axis becomes a vacancy), one labelling
(Device.find_clusters, metal + vacancy members) and on its labels `warmup_calls` untimed and `calls` timed analyses at `slack`, each bracketed by
HIP events on the library's stream, with the library's own split (dkmc_debug_get_path_times under dkmc_set_profiling(1): seeding + search rounds
with their read-backs / summaries); then the host route it replaces -- labels and index copied to the host + tests/path_ref.py there (a
breadth-first search in numpy) -- and a comparison of the two results.
One JSON line per workload and state in <out-dir>/paths_by_size.jsonl.
usage: python tools/time_paths.py [7.5nm tile:10 tile:20] [--slack 2] [--calls 12] [--warmup-calls 3] [--steps 5] [--warmup 2] [--out-dir profiles]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT_NAME = "paths_by_size.jsonl"


def spread(v):
    return dict(median=round(statistics.median(v), 6), min=round(min(v), 6), max=round(max(v), 6), n=len(v))


def child(name, slack, calls, warmup_calls, steps, warmup, out_dir):
    import numpy as np
    import torch
    import cluster_ref as cr
    import path_ref as pr
    from bench import Sim
    from devicekmc_amd import host, lib
    L = lib.load()
    sim = Sim(name, "cuda:0", solve_current=False)
    for _ in range(warmup):
        sim.step(False)
    step_ms = [1e3 * sim.step(True) for _ in range(steps)]
    dev, gb, p = sim.dev, sim.gb, sim.p
    nl, nr = dev.contact_seeds()
    el0 = gb.site_element.cpu().numpy()
    planted, n_planted = cr.plant_filament(el0, dev.site_x, dev.site_y, dev.site_z, 3.0)
    ms2 = (C.c_double * 2)()
    for state, el in (("pristine", el0), ("planted", planted)):
        gb.site_element.copy_(torch.as_tensor(el))
        label, _, cinfo = host.find_clusters(gb.neigh_idx, gb.nn_, gb.site_element, gb.site_charge, gb.site_x, gb.metal_types,
                                             host.METAL | host.VACANCY, nl, nr, capacity=0)
        L.dkmc_set_profiling(1)
        total, lab, summ = [], [], []
        try:
            for i in range(warmup_calls + calls):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                res = host.find_paths(gb.neigh_idx, gb.nn_, label, gb.site_x, nl, nr, slack)
                b.record(); b.synchronize()
                lib.check(L.dkmc_debug_get_path_times(ms2))
                if i >= warmup_calls:
                    total.append(a.elapsed_time(b)); lab.append(ms2[0]); summ.append(ms2[1])
        finally:
            L.dkmc_set_profiling(0)
        # the host route: labels and index to the host, the reference there
        host_ms = []
        for _ in range(3 if dev.N < 2000000 else 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h_label, h_index = label.cpu().numpy(), gb.neigh_idx.cpu().numpy().reshape(dev.N, -1)
            ref = pr.analyse(h_index, h_label, dev.site_x, nl, nr, slack)
            host_ms.append(1e3 * (time.perf_counter() - t0))
        hl, hr, path, prof, info = res
        same = bool(np.array_equal(hl.cpu().numpy(), ref[0]) and np.array_equal(hr.cpu().numpy(), ref[1]) and np.array_equal(path, ref[2])
                    and all(np.array_equal(prof[k], ref[3][k]) for k in pr.PROFILE) and all(info[k] == ref[4][k] for k in pr.INFO))
        t_med, s_med, h_med = statistics.median(total), statistics.median(step_ms), statistics.median(host_ms)
        rec = dict(workload=name, state=state, sites=int(dev.N), nn=int(gb.nn_), members=cinfo["n_members"], planted_sites=n_planted if state == "planted" else 0,
                   slack=slack, **{k: info[k] for k in pr.INFO}, equals_host_reference=same,
                   analysis_ms=spread(total), labelling_ms=spread(lab), summaries_ms=spread(summ),
                   ms_per_round=round(statistics.median(lab) / max(info["rounds"], 1), 6),
                   step_current_off_ms=spread(step_ms), host_route_ms=spread(host_ms),
                   ratio_to_step=round(t_med / s_med, 4), ratio_to_host_route=round(t_med / h_med, 6),
                   dominant_part="labelling" if statistics.median(lab) >= statistics.median(summ) else "summaries")
        line = json.dumps(rec)
        with open(os.path.join(out_dir, OUT_NAME), "a") as f:
            f.write(line + "\n")
        print(line, flush=True)
    gb.site_element.copy_(torch.as_tensor(el0))
    sim.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=["7.5nm", "tile:10", "tile:20"])
    ap.add_argument("--slack", type=int, default=2)
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--warmup-calls", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--append", action="store_true", help="keep the records already in the output file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.slack, a.calls, a.warmup_calls, a.steps, a.warmup, a.out_dir)
    os.makedirs(a.out_dir, exist_ok=True)
    if not a.append:
        open(os.path.join(a.out_dir, OUT_NAME), "w").close()
    bad = 0
    for name in a.workloads:      # one process per workload: every workload starts from a fresh library and allocator
        rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--child", name, "--slack", str(a.slack), "--calls", str(a.calls),
                              "--warmup-calls", str(a.warmup_calls), "--steps", str(a.steps), "--warmup", str(a.warmup), "--out-dir", a.out_dir])
        if rc:
            print("%s: child ended with %d" % (name, rc), file=sys.stderr)
            bad = 1
            break                 # nothing more is started on the GPU after a failure
    sys.exit(bad)


if __name__ == "__main__":
    main()
