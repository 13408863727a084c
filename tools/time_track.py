#!/usr/bin/env python3
"""What the cluster tracking (dkmc_track_clusters) costs, against the two things it is measured by.  One child process per workload.  In it: a
simulation with the current solve off, a labelling of the pristine device (Device.find_clusters, metal + vacancy members), `warmup` untimed and
`steps` timed supersteps (the step the analysis would follow) and a labelling after them; then two labellings of the same device with the planted
filament of the tests, open (every O site within 3 A of the axis becomes a vacancy, 25 < x < 40 left out) and bridged (all of them).  On either
pair of labellings -- "steps": pristine -> after the supersteps, "planted": open -> bridged -- `warmup_calls` untimed and `calls` timed analyses,
each bracketed by HIP events on the library's stream, with the library's own split (dkmc_debug_get_track_times under dkmc_set_profiling(1): the
pair pass / everything after it); then the host route it replaces -- both label arrays copied to the host and np.unique over the pairs there --
and a comparison of the device result with tests/track_ref.py.
One JSON line per workload and state in <out-dir>/track_by_size.jsonl.
usage: python tools/time_track.py [7.5nm tile:10 tile:20] [--calls 12] [--warmup-calls 3] [--steps 5] [--warmup 2] [--out-dir profiles]"""
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

OUT_NAME = "track_by_size.jsonl"


def spread(v):
    return dict(median=round(statistics.median(v), 6), min=round(min(v), 6), max=round(max(v), 6), n=len(v))


def host_route(label_prev, label_now):
    """both label arrays to the host, the distinct pairs with their counts and first sites there"""
    import numpy as np
    lp, ln = label_prev.cpu().numpy().astype(np.int64), label_now.cpu().numpy().astype(np.int64)
    N = len(lp)
    a, b = np.where((lp >= 0) & (lp < N), lp, -1), np.where((ln >= 0) & (ln < N), ln, -1)
    ids = np.flatnonzero((a >= 0) | (b >= 0))
    return np.unique((a[ids] + 1) * (N + 1) + (b[ids] + 1), return_index=True, return_counts=True)


def child(name, calls, warmup_calls, steps, warmup, out_dir):
    import numpy as np
    import torch
    import cluster_ref as cr
    import track_ref as tr
    from bench import Sim
    from devicekmc_amd import host, lib
    L = lib.load()
    sim = Sim(name, "cuda:0", solve_current=False)
    dev, gb, p = sim.dev, sim.gb, sim.p
    nl, nr = dev.contact_seeds()

    def labelling():
        label, _, info = host.find_clusters(gb.neigh_idx, gb.nn_, gb.site_element, gb.site_charge, gb.site_x, gb.metal_types,
                                            host.METAL | host.VACANCY, nl, nr, capacity=0)
        return label, info

    el0 = gb.site_element.cpu().numpy()
    pristine = labelling()
    for _ in range(warmup):
        sim.step(False)
    step_ms = [1e3 * sim.step(True) for _ in range(steps)]
    after = labelling()
    el1 = gb.site_element.cpu().numpy()
    planted = []
    for skip in ((25.0, 40.0), None):
        gb.site_element.copy_(torch.as_tensor(cr.plant_filament(el0, dev.site_x, dev.site_y, dev.site_z, 3.0, skip)[0]))
        planted.append(labelling())
    gb.site_element.copy_(torch.as_tensor(el1))
    ms2 = (C.c_double * 2)()
    for state, (lp, ip), (ln, inow) in (("steps", pristine, after), ("planted", planted[0], planted[1])):
        L.dkmc_set_profiling(1)
        total, pair_ms, rest_ms = [], [], []
        try:
            for i in range(warmup_calls + calls):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                res = host.track_clusters(lp, ln, gb.site_x, nl, nr)
                b.record(); b.synchronize()
                lib.check(L.dkmc_debug_get_track_times(ms2))
                if i >= warmup_calls:
                    total.append(a.elapsed_time(b)); pair_ms.append(ms2[0]); rest_ms.append(ms2[1])
        finally:
            L.dkmc_set_profiling(0)
        # the host route: both label arrays to the host, np.unique over the pairs there
        host_ms = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            keys, _, _ = host_route(lp, ln)
            host_ms.append(1e3 * (time.perf_counter() - t0))
        change, pairs, now, prev, critical, info = res
        ref = tr.analyse(lp.cpu().numpy(), ln.cpu().numpy(), dev.site_x, nl, nr)
        try:
            tr.assert_equal(change.cpu().numpy(), pairs, now, prev, critical, info, ref)
            same = len(keys) == info["n_pairs"]
        except AssertionError:
            same = False
        t_med, s_med, h_med = statistics.median(total), statistics.median(step_ms), statistics.median(host_ms)
        rec = dict(workload=name, state=state, sites=int(dev.N), members_prev=ip["n_members"], members_now=inow["n_members"],
                   **{k: info[k] for k in tr.INFO}, equals_host_reference=bool(same),
                   analysis_ms=spread(total), pair_pass_ms=spread(pair_ms), rest_ms=spread(rest_ms),
                   step_current_off_ms=spread(step_ms), host_route_ms=spread(host_ms),
                   ratio_to_step=round(t_med / s_med, 4), ratio_to_host_route=round(t_med / h_med, 6),
                   dominant_part="pair pass" if statistics.median(pair_ms) >= statistics.median(rest_ms) else "rest")
        line = json.dumps(rec)
        with open(os.path.join(out_dir, OUT_NAME), "a") as f:
            f.write(line + "\n")
        print(line, flush=True)
    sim.close()


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
