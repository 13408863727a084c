#!/usr/bin/env python3
"""What the min-cut analysis (dkmc_find_flow) costs, against the things it is measured by.  One child process per workload.  In it: a simulation
with the current solve off, `warmup` untimed and `steps` timed supersteps (the step the analysis would follow); then, on the same device in its
pristine state (radius 0) and with a planted bridging filament at each other radius (every O site within r of the axis becomes a vacancy), one
labelling (Device.find_clusters, metal + vacancy members) and one path search (find_paths, slack 0), both timed the same way for the comparison,
and on their labels `warmup_calls` untimed and `calls` timed analyses, each bracketed by HIP events on the library's stream, with the library's
own split (dkmc_debug_get_flow_times under dkmc_set_profiling(1): strand searches with their predecessor passes and one-thread walks / the two
closing searches / tables and copy-out); then the host route it replaces -- labels and index copied to the host + a maximum flow on the
vertex-split graph there (scipy.sparse.csgraph.maximum_flow where scipy is installed, else tests/flow_ref.py) -- and a comparison of W.
One JSON line per workload and radius in <out-dir>/flow_by_size.jsonl.
With --trace the child only plants the LAST radius and makes `calls` analyses: the run to put under `rocprofv3 --kernel-trace --stats`, whose
per-kernel table gives the share of the one-thread walks (k_fl_walk) that HIP events on the stream cannot separate.
usage: python tools/time_flow.py [7.5nm tile:10 tile:20] [--radii 0 2.2 4.5] [--calls 12] [--warmup-calls 3] [--steps 5] [--warmup 2]
       [--max-strands 64] [--out-dir profiles] [--append] [--trace]"""
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

OUT_NAME = "flow_by_size.jsonl"


def spread(v):
    return dict(median=round(statistics.median(v), 6), min=round(min(v), 6), max=round(max(v), 6), n=len(v))


def host_max_flow(index, label, n_left, n_right):
    """-> (W, -1 where the contacts touch; the method's name): the value of a maximum flow on the vertex-split graph of the members"""
    import numpy as np
    import flow_ref as fl
    try:
        from scipy.sparse import csr_matrix
        from scipy.sparse.csgraph import maximum_flow
    except ImportError:
        return fl.analyse(index, label, None, n_left, n_right, max_strands=4096)[4]["width"], "tests/flow_ref.py"
    mask, ptr, nb, sl, sr = fl.graph(index, label, n_left, n_right)
    N = len(mask)
    interior = mask & ~sl & ~sr
    u = np.repeat(np.arange(N), np.diff(ptr))
    if (sl & sr).any() or (sl[u] & sr[nb]).any():
        return -1, "scipy.sparse.csgraph.maximum_flow"
    rank = np.cumsum(interior) - 1
    n_in = int(interior.sum())
    both = interior[u] & interior[nb]
    near_l, near_r = np.unique(nb[sl[u] & interior[nb]]), np.unique(nb[sr[u] & interior[nb]])
    r_all = np.arange(n_in)
    rows = np.concatenate([2 + 2 * r_all, 3 + 2 * rank[u[both]], np.zeros(len(near_l), dtype=np.int64), 3 + 2 * rank[near_r]])
    cols = np.concatenate([3 + 2 * r_all, 2 + 2 * rank[nb[both]], 2 + 2 * rank[near_l], np.ones(len(near_r), dtype=np.int64)])
    g = csr_matrix((np.ones(len(rows), dtype=np.int32), (rows, cols)), shape=(2 + 2 * n_in, 2 + 2 * n_in))
    return int(maximum_flow(g, 0, 1).flow_value), "scipy.sparse.csgraph.maximum_flow"


def child(name, radii, calls, warmup_calls, steps, warmup, max_strands, out_dir, trace):
    import torch
    import cluster_ref as cr
    from bench import Sim
    from devicekmc_amd import host, lib
    L = lib.load()
    sim = Sim(name, "cuda:0", solve_current=False)
    step_ms = []
    if not trace:
        for _ in range(warmup):
            sim.step(False)
        step_ms = [1e3 * sim.step(True) for _ in range(steps)]
    dev, gb, p = sim.dev, sim.gb, sim.p
    nl, nr = dev.contact_seeds()
    el0 = gb.site_element.cpu().numpy()
    ms3 = (C.c_double * 3)()

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

    for r in (radii[-1:] if trace else radii):
        planted, n_planted = cr.plant_filament(el0, dev.site_x, dev.site_y, dev.site_z, r) if r > 0 else (el0, 0)
        gb.site_element.copy_(torch.as_tensor(planted))
        cl_ms, (label, _, cinfo) = timed(lambda: host.find_clusters(gb.neigh_idx, gb.nn_, gb.site_element, gb.site_charge, gb.site_x, gb.metal_types,
                                                                    host.METAL | host.VACANCY, nl, nr, capacity=0), warmup_calls, calls)
        flow = lambda: host.find_flow(gb.neigh_idx, gb.nn_, label, gb.site_x, nl, nr, max_strands)
        if trace:
            for _ in range(calls):
                info = flow()[4]
            print(json.dumps(dict(workload=name, radius=r, sites=int(dev.N), calls=calls, **{k: info[k] for k in host.FLOW_INFO})), flush=True)
            continue
        pt_ms, (_, _, _, _, pinfo) = timed(lambda: host.find_paths(gb.neigh_idx, gb.nn_, label, gb.site_x, nl, nr, 0), warmup_calls, calls)
        L.dkmc_set_profiling(1)
        total, parts = [], ([], [], [])
        try:
            for i in range(warmup_calls + calls):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                res = flow()
                b.record(); b.synchronize()
                lib.check(L.dkmc_debug_get_flow_times(ms3))
                if i >= warmup_calls:
                    total.append(a.elapsed_time(b))
                    for k in range(3):
                        parts[k].append(ms3[k])
        finally:
            L.dkmc_set_profiling(0)
        info = res[4]
        # the host route: labels and index to the host, a maximum flow there
        host_ms = []
        for _ in range(3 if dev.N < 2000000 else 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h_label, h_index = label.cpu().numpy(), gb.neigh_idx.cpu().numpy().reshape(dev.N, -1)
            w_host, method = host_max_flow(h_index, h_label, nl, nr)
            host_ms.append(1e3 * (time.perf_counter() - t0))
        t_med, s_med, h_med, p_med = statistics.median(total), statistics.median(step_ms), statistics.median(host_ms), statistics.median(pt_ms)
        rec = dict(workload=name, radius=r, sites=int(dev.N), nn=int(gb.nn_), members=cinfo["n_members"], planted_sites=n_planted,
                   bridged=cinfo["bridged"], hops=pinfo["hops"], max_strands=max_strands, **{k: info[k] for k in host.FLOW_INFO},
                   cut_left_x=[info["cut_left_xmin"], info["cut_left_xmax"]] if info["status"] == 1 else None,
                   cut_right_x=[info["cut_right_xmin"], info["cut_right_xmax"]] if info["status"] == 1 else None,
                   host_route=method, host_route_width=w_host, width_equals_host_route=bool(w_host == info["width"]),
                   analysis_ms=spread(total), strand_searches_ms=spread(parts[0]), closing_searches_ms=spread(parts[1]), tables_ms=spread(parts[2]),
                   find_clusters_ms=spread(cl_ms), find_clusters_rounds=cinfo["rounds"], find_paths_ms=spread(pt_ms), find_paths_rounds=pinfo["rounds"],
                   step_current_off_ms=spread(step_ms), host_route_ms=spread(host_ms),
                   ratio_to_step=round(t_med / s_med, 4), ratio_to_host_route=round(t_med / h_med, 6),
                   ratio_to_find_clusters=round(t_med / statistics.median(cl_ms), 4), ratio_to_find_paths=round(t_med / p_med, 4),
                   find_paths_calls_per_search=round(t_med / p_med / max(info["searches"], 1), 4),
                   ms_per_round=round(t_med / max(info["rounds"], 1), 6))
        line = json.dumps(rec)
        with open(os.path.join(out_dir, OUT_NAME), "a") as f:
            f.write(line + "\n")
        print(line, flush=True)
    gb.site_element.copy_(torch.as_tensor(el0))
    sim.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=["7.5nm", "tile:10", "tile:20"])
    ap.add_argument("--radii", type=float, nargs="+", default=[0.0, 2.2, 4.5], help="0: the pristine cell")
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--warmup-calls", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-strands", type=int, default=64)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--append", action="store_true", help="keep the records already in the output file")
    ap.add_argument("--trace", action="store_true", help="only the analyses of the last radius: the run for a kernel trace; writes no record")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.radii, a.calls, a.warmup_calls, a.steps, a.warmup, a.max_strands, a.out_dir, a.trace)
    if a.trace:                   # in this process: the profiler follows no child
        for name in a.workloads:
            child(name, a.radii, a.calls, a.warmup_calls, a.steps, a.warmup, a.max_strands, a.out_dir, True)
        return
    os.makedirs(a.out_dir, exist_ok=True)
    if not a.append:
        open(os.path.join(a.out_dir, OUT_NAME), "w").close()
    bad = 0
    for name in a.workloads:      # one process per workload: every workload starts from a fresh library and allocator
        rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--child", name, "--radii"] + [str(r) for r in a.radii] +
                             ["--calls", str(a.calls), "--warmup-calls", str(a.warmup_calls), "--steps", str(a.steps), "--warmup", str(a.warmup),
                              "--max-strands", str(a.max_strands), "--out-dir", a.out_dir])
        if rc:
            print("%s: child ended with %d" % (name, rc), file=sys.stderr)
            bad = 1
            break                 # nothing more is started on the GPU after a failure
    sys.exit(bad)


if __name__ == "__main__":
    main()
