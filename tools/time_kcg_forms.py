#!/usr/bin/env python3
"""The CG on K on its CSR positions (default above 262 144 rows) against the windowed blocked form (dkmc_set_k_blocked_large(1)) with 4-byte and with
2-byte stored words (dkmc_set_k_window_word_bytes), on the same workloads with the current solve off; the 4-byte case runs twice (first and last), so
that the run-to-run spread of the reference point is on record.  Per case one background-potential solve from the Laplace start at the library's default tolerance (iterations,
HIP-event time of the iteration loop per iteration: kcg_ms / kcg_iters_timed) and the superstep rate (charge + potential + events) over `steps`
supersteps after one untimed one; for the windowed form the window and segment statistics of the build (dkmc_kcg_form_info).  The product's own
launch time comes from a rocprofv3 --kernel-trace --stats run of this script (k_kc_apply against k_kbw_apply<0, 4> and k_kbw_apply<0, 2>).
usage: python tools/time_kcg_forms.py [tile:20 tile:10 ...] [--steps 3]"""
import argparse
import ctypes as C
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Vd = 5.0


def run(name, large, word_bytes, steps):
    import torch
    from bench import make_workload
    from devicekmc_amd import host, lib
    L = lib.load()
    L.dkmc_set_k_blocked_large(large); L.dkmc_set_k_window_word_bytes(word_bytes)
    try:
        s, p = make_workload(name)
        p.solve_current = False; p.solve_heating_global = False
        t0 = time.perf_counter()
        dev = host.Device(s, p, gpu_neighbors="cuda:0")
        sim = host.KMCProcess(dev, p.freq)
        gb = dev.make_gpubuf("cuda:0")
        dev.setLaplacePotential(gb, p, Vd)
        gb.sync_HostToGPU(dev)
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0
        info = (C.c_longlong * 9)()
        lib.check(L.dkmc_kcg_form_info(C.byref(gb.c), info))
        words = (C.c_longlong * 3)()
        lib.check(L.dkmc_kcg_form_words(C.byref(gb.c), words))
        dev.updateCharge(gb)
        L.dkmc_set_profiling(1)
        dev.updatePotential(gb, p, Vd, 0)
        torch.cuda.synchronize()
        L.dkmc_set_profiling(0)
        st = host.get_stats()
        out = dict(workload=name, sites=int(s.N), form=int(st["kcg_blocked"]), K_rows=int(info[1]), build_s=round(build_s, 2),
                   iters=int(st["cg_iters_K"]), loop_ms=round(st["kcg_ms"], 3), us_per_iter=round(1e3 * st["kcg_ms"] / max(1, st["kcg_iters_timed"]), 2),
                   kcg_bytes_per_iter=int(st["kcg_bytes"]))
        if info[0] == 2:
            f, rows, R, nb, maxwin, winsum, maxseg, segsum, ints = list(info)
            out.update(rows_per_block=R, blocks=nb, window_max=maxwin, window_mean=round(winsum / nb, 1), window_over_rows=round(winsum / rows, 3),
                       segments_max=maxseg, segments_mean=round(segsum / nb, 2), stored_ints=ints, stored_ints_per_row=round(ints / rows, 2),
                       word_bytes=int(words[0]), word_bytes_total=int(words[2]))
        _, dt = sim.executeKMCStep(gb, dev)
        k = 1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, k)
            sim.executeKMCStep(gb, dev)
            k += 1
        torch.cuda.synchronize()
        out["steps_per_s"] = round(steps / (time.perf_counter() - t0), 3)
        out["iters_last_step"] = int(host.get_stats()["cg_iters_K"])
        del gb, sim, dev
        torch.cuda.empty_cache()
        return out
    finally:
        L.dkmc_set_k_blocked_large(0); L.dkmc_set_k_window_word_bytes(4); L.dkmc_set_profiling(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=["tile:20", "tile:10"])
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    for name in a.workloads:
        for large, word_bytes in ((1, 4), (0, 4), (1, 2), (1, 4)):
            print(json.dumps(run(name, large, word_bytes, a.steps)), flush=True)


if __name__ == "__main__":
    main()
