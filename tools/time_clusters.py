#!/usr/bin/env python3
"""What the filament analysis (dkmc_find_clusters) costs, against the two things it is measured by.  One child process per workload.  In it:
a simulation with the current solve off, `warmup` untimed and `steps` timed supersteps (the step the analysis would gate); then on that state
`warmup_calls` untimed and `calls` timed analyses (metal + vacancy members over neigh_idx, default contact seeds), each bracketed by HIP events on
the library's stream, with the library's own split (dkmc_debug_get_cluster_times under dkmc_set_profiling(1): membership + labelling rounds with
their read-backs / summaries); then the host route it replaces -- site_element copied to the host + tests/cluster_ref.py there -- and a
comparison of the two results.  The byte floor is one read of the member rows of the index at the rate the project's streaming kernel reaches
(k_xtb_apply: 5.85-6.11 TB/s), per round and for the rounds run.
One JSON line per workload in <out-dir>/clusters_by_size.jsonl.
usage: python tools/time_clusters.py [7.5nm tile:10 tile:20] [--calls 12] [--warmup-calls 3] [--steps 5] [--warmup 2] [--out-dir profiles]"""
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

OUT_NAME = "clusters_by_size.jsonl"
STREAM_TBS = 6.0


def spread(v):
    return dict(median=round(statistics.median(v), 6), min=round(min(v), 6), max=round(max(v), 6), n=len(v))


def child(name, calls, warmup_calls, steps, warmup, out_dir):
    import numpy as np
    import torch
    import cluster_ref as cr
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

    def analyse():
        return host.find_clusters(gb.neigh_idx, gb.nn_, gb.site_element, gb.site_charge, gb.site_x, gb.metal_types, members, nl, nr, capacity=0)

    L.dkmc_set_profiling(1)
    total, lab, summ = [], [], []
    ms2 = (C.c_double * 2)()
    try:
        for i in range(warmup_calls + calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            label, _, info = analyse()
            b.record(); b.synchronize()
            lib.check(L.dkmc_debug_get_cluster_times(ms2))
            if i >= warmup_calls:
                total.append(a.elapsed_time(b)); lab.append(ms2[0]); summ.append(ms2[1])
    finally:
        L.dkmc_set_profiling(0)
    # the host route: the element array to the host, the reference there (its model of the rounds left out: only the result is wanted)
    host_ms = []
    for _ in range(3 if dev.N < 2000000 else 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        el = gb.site_element.cpu().numpy()
        ref = cr.analyse(dev.neigh_idx, el, None, dev.site_x, list(p.metals), members, nl, nr, with_rounds=False)
        host_ms.append(1e3 * (time.perf_counter() - t0))
    same = bool(np.array_equal(label.cpu().numpy(), ref[0]) and all(info[k] == ref[2][k] for k in ref[2]))
    t_med, s_med, h_med = statistics.median(total), statistics.median(step_ms), statistics.median(host_ms)
    row_bytes = 4 * int(gb.nn_) * info["n_members"]
    floor_round_ms = row_bytes / (STREAM_TBS * 1e12) * 1e3
    rec = dict(workload=name, sites=int(dev.N), nn=int(gb.nn_), members=info["n_members"], components=info["n_components"], rounds=info["rounds"],
               bridged=info["bridged"], equals_host_reference=same,
               analysis_ms=spread(total), labelling_ms=spread(lab), summaries_ms=spread(summ),
               step_current_off_ms=spread(step_ms), host_route_ms=spread(host_ms),
               member_row_bytes_per_round=row_bytes, stream_rate_TBs=STREAM_TBS, floor_one_round_ms=round(floor_round_ms, 6),
               floor_rounds_ms=round(floor_round_ms * info["rounds"], 6),
               ratio_to_step=round(t_med / s_med, 4), ratio_to_host_route=round(t_med / h_med, 6),
               ratio_to_floor_one_round=round(t_med / floor_round_ms, 1), ratio_to_floor_rounds=round(t_med / (floor_round_ms * info["rounds"]), 1),
               dominant_part="labelling" if statistics.median(lab) >= statistics.median(summ) else "summaries")
    sim.close()
    line = json.dumps(rec)
    with open(os.path.join(out_dir, OUT_NAME), "a") as f:
        f.write(line + "\n")
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=["7.5nm", "tile:10", "tile:20"])
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--warmup-calls", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--append", action="store_true", help="keep the records already in the output file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.calls, a.warmup_calls, a.steps, a.warmup, a.out_dir)
    os.makedirs(a.out_dir, exist_ok=True)
    if not a.append:
        open(os.path.join(a.out_dir, OUT_NAME), "w").close()
    bad = 0
    for name in a.workloads:      # one process per workload: every workload starts from a fresh library and allocator
        rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--child", name, "--calls", str(a.calls), "--warmup-calls", str(a.warmup_calls),
                              "--steps", str(a.steps), "--warmup", str(a.warmup), "--out-dir", a.out_dir])
        if rc:
            print("%s: child ended with %d" % (name, rc), file=sys.stderr)
            bad = 1
            break                 # nothing more is started on the GPU after a failure
    sys.exit(bad)


if __name__ == "__main__":
    main()
