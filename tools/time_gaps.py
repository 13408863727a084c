#!/usr/bin/env python3
"""What the gap analysis (dkmc_find_gaps) costs, beside the two things it is measured by.  One child process per workload.  In it: a simulation
with the current solve off, `warmup` untimed and `steps` timed supersteps; then on that state one find_clusters (metal + vacancy members over
neigh_idx) whose labels every analysis below reads; for every r_max, with the uniform-cell skip on and off, `warmup_calls` untimed and `calls`
timed analyses, each bracketed by HIP events on the library's stream; and the route available without it for ONE probe radius: a neighbour index
built on the device at radius r_max (dkmc_build_neighbor_index, both of its calls, on the device's coordinate arrays) + dkmc_find_clusters over it.
A bisection for the bottleneck pays that route once per probe.  The route is left out -- with the reason in the record -- where its index alone
would exceed --route-max-gib.  The two settings of the skip are also compared result by result.
One JSON line per workload and r_max in <out-dir>/gaps_by_size.jsonl.
usage: python tools/time_gaps.py [7.5nm tile:10 tile:20] [--r-max 6 10 16] [--calls 8] [--warmup-calls 2] [--steps 5] [--warmup 2] [--out-dir profiles]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT_NAME = "gaps_by_size.jsonl"


def spread(v):
    return dict(median=round(statistics.median(v), 6), min=round(min(v), 6), max=round(max(v), 6), n=len(v))


def child(name, radii, calls, warmup_calls, steps, warmup, route_max_gib, out_dir):
    import numpy as np
    import torch
    from bench import Sim
    from devicekmc_amd import host, lib
    L = lib.load()
    sim = Sim(name, "cuda:0", solve_current=False)
    for _ in range(warmup):
        sim.step(False)
    step_ms = [1e3 * sim.step(True) for _ in range(steps)]
    dev, gb, p = sim.dev, sim.gb, sim.p
    nl, nr = dev.contact_seeds()
    members = host.METAL | host.VACANCY
    label, _, cinfo = host.find_clusters(gb.neigh_idx, gb.nn_, gb.site_element, gb.site_charge, gb.site_x, gb.metal_types, members, nl, nr, capacity=0)
    lat = np.ascontiguousarray(p.lattice, dtype=np.float64)

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

    def route(r):
        """the index at radius r, then the components over it"""
        nn = C.c_int(0)
        xyz = (host._ptr(gb.site_x), host._ptr(gb.site_y), host._ptr(gb.site_z), host._np_ptr(lat), int(p.pbc), float(r))
        lib.check(L.dkmc_build_neighbor_index(dev.N, *xyz, C.byref(nn), None))
        index = torch.empty(dev.N * nn.value, dtype=torch.int32, device=gb.dev)
        lib.check(L.dkmc_build_neighbor_index(dev.N, *xyz, C.byref(nn), host._ptr(index)))
        _, _, info = host.find_clusters(index, nn.value, gb.site_element, gb.site_charge, gb.site_x, gb.metal_types, members, nl, nr, capacity=0)
        return nn.value, info

    density = dev.N / ((dev.site_x.max() - dev.site_x.min()) * (dev.site_y.max() - dev.site_y.min()) * (dev.site_z.max() - dev.site_z.min()))
    for r in radii:
        rec = dict(workload=name, sites=int(dev.N), members=cinfo["n_members"], r_max=r, step_current_off_ms=spread(step_ms))
        results = {}
        for skip in (1, 0):
            L.dkmc_debug_set_gap_cell_skip(skip)
            ms, results[skip] = timed(lambda: host.find_gaps(label, gb.site_x, gb.site_y, gb.site_z, p.lattice, p.pbc, nl, nr, r), warmup_calls, calls)
            rec["analysis_ms_skip_%s" % ("on" if skip else "off")] = spread(ms)
            rec["pairs_tested_skip_%s" % ("on" if skip else "off")] = results[skip][2]["pairs_tested"]
        L.dkmc_debug_set_gap_cell_skip(1)
        (e1, c1, i1), (e0, c0, i0) = results[1], results[0]
        rec["skip_on_equals_off"] = bool(all(np.array_equal(e1[k], e0[k]) for k in e1) and all(np.array_equal(c1[k], c0[k]) for k in c1)
                                         and all(i1[k] == i0[k] for k in i1 if k != "pairs_tested"))
        rec.update({k: i1[k] for k in ("n_components", "n_edges", "status", "n_hops", "rounds", "bottleneck")})
        rec["direct"] = None if i1["direct"] is None else i1["direct"][2]
        rec["bottleneck"] = rec["bottleneck"] if np.isfinite(rec["bottleneck"]) else None
        est_gib = dev.N * density * 4.19 * r ** 3 * 4 / 2 ** 30
        if est_gib > route_max_gib:
            rec["route_ms"], rec["route_note"] = None, "not measured: an index of about %.0f GiB (limit %.0f)" % (est_gib, route_max_gib)
        else:
            big = est_gib > 1.0
            ms, (nn, rinfo) = timed(lambda: route(r), 0 if big else 1, 1 if big else 3)
            rec["route_ms"], rec["route_nn"], rec["route_bridged"] = spread(ms), nn, rinfo["bridged"]
            rec["ratio_to_route"] = round(rec["analysis_ms_skip_on"]["median"] / statistics.median(ms), 6)
        rec["ratio_to_step"] = round(rec["analysis_ms_skip_on"]["median"] / statistics.median(step_ms), 4)
        rec["skip_off_over_on"] = round(rec["analysis_ms_skip_off"]["median"] / rec["analysis_ms_skip_on"]["median"], 4)
        line = json.dumps(rec)
        with open(os.path.join(out_dir, OUT_NAME), "a") as f:
            f.write(line + "\n")
        print(line, flush=True)
    sim.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=["7.5nm", "tile:10", "tile:20"])
    ap.add_argument("--r-max", type=float, nargs="+", default=[6.0, 10.0, 16.0])
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--warmup-calls", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--route-max-gib", type=float, default=12.0, help="largest neighbour index the comparison route may build")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--append", action="store_true", help="keep the records already in the output file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.r_max, a.calls, a.warmup_calls, a.steps, a.warmup, a.route_max_gib, a.out_dir)
    os.makedirs(a.out_dir, exist_ok=True)
    if not a.append:
        open(os.path.join(a.out_dir, OUT_NAME), "w").close()
    bad = 0
    for name in a.workloads:      # one process per workload: every workload starts from a fresh library and allocator
        rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--child", name, "--r-max"] + [str(r) for r in a.r_max] +
                             ["--calls", str(a.calls), "--warmup-calls", str(a.warmup_calls), "--steps", str(a.steps), "--warmup", str(a.warmup),
                              "--route-max-gib", str(a.route_max_gib), "--out-dir", a.out_dir])
        if rc:
            print("%s: child ended with %d" % (name, rc), file=sys.stderr)
            bad = 1
            break                 # nothing more is started on the GPU after a failure
    sys.exit(bad)


if __name__ == "__main__":
    main()
