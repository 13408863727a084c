#!/usr/bin/env python3
"""What the cut-site analysis (dkmc_find_cuts) costs, against the things it is measured by.  One child process per workload.  In it: a simulation
with the current solve off, `warmup` untimed and `steps` timed supersteps (the step the analysis would follow); then, on the same device with a
planted bridging filament at each radius (every O site within r of the axis becomes a vacancy), one labelling (Device.find_clusters, metal +
vacancy members) and one path search (find_paths, slack 0), both timed the same way for the comparison, and on their labels and path
`warmup_calls` untimed and `calls` timed analyses, each bracketed by HIP events on the library's stream, with the library's own split
(dkmc_debug_get_cut_times under dkmc_set_profiling(1): off-path labelling rounds with their read-backs / everything else); then the host route it
replaces -- labels, index and path copied to the host + tests/cut_ref.py there -- and a comparison of the two results.
One JSON line per workload and radius in <out-dir>/cuts_by_size.jsonl.
usage: python tools/time_cuts.py [7.5nm tile:10 tile:20] [--radii 3.0 2.2] [--calls 12] [--warmup-calls 3] [--steps 5] [--warmup 2] [--out-dir profiles]"""
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

OUT_NAME = "cuts_by_size.jsonl"


def spread(v):
    return dict(median=round(statistics.median(v), 6), min=round(min(v), 6), max=round(max(v), 6), n=len(v))


def child(name, radii, calls, warmup_calls, steps, warmup, out_dir):
    import numpy as np
    import torch
    import cluster_ref as cr
    import cut_ref as cu
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
    ms2 = (C.c_double * 2)()

    def timed(fn, n_warm, n):
        out, res = [], None
        for i in range(n_warm + n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            res = fn()
            b.record(); b.synchronize()
            if i >= n_warm:
                out.append(a.elapsed_time(b))
        return out, res

    for r in radii:
        planted, n_planted = cr.plant_filament(el0, dev.site_x, dev.site_y, dev.site_z, r)
        gb.site_element.copy_(torch.as_tensor(planted))
        cl_ms, (label, _, cinfo) = timed(lambda: host.find_clusters(gb.neigh_idx, gb.nn_, gb.site_element, gb.site_charge, gb.site_x, gb.metal_types,
                                                                    host.METAL | host.VACANCY, nl, nr, capacity=0), warmup_calls, calls)
        pt_ms, (_, _, path, _, pinfo) = timed(lambda: host.find_paths(gb.neigh_idx, gb.nn_, label, gb.site_x, nl, nr, 0), warmup_calls, calls)
        d_path = torch.as_tensor(path).to("cuda:0")
        L.dkmc_set_profiling(1)
        total, lab, rest = [], [], []
        try:
            for i in range(warmup_calls + calls):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                res = host.find_cuts(gb.neigh_idx, gb.nn_, label, gb.site_x, nl, nr, d_path)
                b.record(); b.synchronize()
                lib.check(L.dkmc_debug_get_cut_times(ms2))
                if i >= warmup_calls:
                    total.append(a.elapsed_time(b)); lab.append(ms2[0]); rest.append(ms2[1])
        finally:
            L.dkmc_set_profiling(0)
        # the host route: labels, index and path to the host, the reference there
        host_ms = []
        for _ in range(3 if dev.N < 2000000 else 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h_label, h_index, h_path = label.cpu().numpy(), gb.neigh_idx.cpu().numpy().reshape(dev.N, -1), d_path.cpu().numpy()
            ref = cu.analyse(h_index, h_label, dev.site_x, nl, nr, h_path)
            host_ms.append(1e3 * (time.perf_counter() - t0))
        role, bypass, table, byp, necks, info = res
        same = bool(np.array_equal(role.cpu().numpy(), ref[0]) and np.array_equal(bypass.cpu().numpy(), ref[1])
                    and all(np.array_equal(table[k], ref[2][k]) for k in cu.PATH) and all(np.array_equal(byp[k], ref[3][k]) for k in cu.BYPASSES)
                    and all(np.array_equal(necks[k], ref[4][k]) for k in cu.NECKS) and all(info[k] == ref[5][k] for k in cu.INFO))
        t_med, s_med, h_med = statistics.median(total), statistics.median(step_ms), statistics.median(host_ms)
        rec = dict(workload=name, radius=r, sites=int(dev.N), nn=int(gb.nn_), members=cinfo["n_members"], planted_sites=n_planted,
                   bridged=cinfo["bridged"], hops=pinfo["hops"], **{k: info[k] for k in cu.INFO}, equals_host_reference=same,
                   analysis_ms=spread(total), labelling_ms=spread(lab), rest_ms=spread(rest),
                   find_clusters_ms=spread(cl_ms), find_clusters_rounds=cinfo["rounds"], find_paths_ms=spread(pt_ms), find_paths_rounds=pinfo["rounds"],
                   step_current_off_ms=spread(step_ms), host_route_ms=spread(host_ms),
                   ratio_to_step=round(t_med / s_med, 4), ratio_to_host_route=round(t_med / h_med, 6),
                   ratio_to_find_clusters=round(t_med / statistics.median(cl_ms), 4), ratio_to_find_paths=round(t_med / statistics.median(pt_ms), 4),
                   dominant_part="labelling" if statistics.median(lab) >= statistics.median(rest) else "rest")
        line = json.dumps(rec)
        with open(os.path.join(out_dir, OUT_NAME), "a") as f:
            f.write(line + "\n")
        print(line, flush=True)
    gb.site_element.copy_(torch.as_tensor(el0))
    sim.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=["7.5nm", "tile:10", "tile:20"])
    ap.add_argument("--radii", type=float, nargs="+", default=[3.0, 2.2])
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--warmup-calls", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--append", action="store_true", help="keep the records already in the output file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.radii, a.calls, a.warmup_calls, a.steps, a.warmup, a.out_dir)
    os.makedirs(a.out_dir, exist_ok=True)
    if not a.append:
        open(os.path.join(a.out_dir, OUT_NAME), "w").close()
    bad = 0
    for name in a.workloads:      # one process per workload: every workload starts from a fresh library and allocator
        rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--child", name, "--radii"] + [str(r) for r in a.radii] +
                             ["--calls", str(a.calls), "--warmup-calls", str(a.warmup_calls), "--steps", str(a.steps), "--warmup", str(a.warmup),
                              "--out-dir", a.out_dir])
        if rc:
            print("%s: child ended with %d" % (name, rc), file=sys.stderr)
            bad = 1
            break                 # nothing more is started on the GPU after a failure
    sys.exit(bad)


if __name__ == "__main__":
    main()
