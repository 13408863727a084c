"""Strong-scaling model of the slab-distributed block-CG with and without the split polynomial preconditioner (dkmc_set_x_slab_poly).  Needs a GPU.

For tile:10 (939 900 sites) and the 85 071-site device (7.5nm): one single-GPU run of the library defaults (preconditioned, d = 8) leaves X resident,
then N = 1, 2, 4, 8 VIRTUAL ranks run the distributed loop on it (dkmc_xtb_emulate_slabs, default tolerance, from a zero start) with the switch off
and on.  Recorded per (N, switch): sweeps to the tolerance (and the one-GPU reference's), per-rank kernel times of the middle rank, the mean N x panel
product time, exchanges per sweep and doubles per halo exchange (dkmc_xtb_slab_last).  The model prices every exchange with the ASSUMED constants of
bench.py's strong_scaling_model_slabs; exchange durations are not measured and nothing here ran on more than one GPU.

    python tools/slab_poly_model.py [--workloads tile:10,7.5nm] [--out profiles/slab_poly_model.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (workloads, Sim, the ASSUMED exchange constants)


def pair_us(doubles, n, peers=None):
    """ASSUMED duration of one all-to-all-v: payload spread over the links to `peers` ranks (default all n - 1) + latency (bench.py's constants)."""
    if n == 1:
        return 0.0
    k = n - 1 if peers is None else max(1, min(peers, n - 1))
    return doubles * 8.0 / k / (bench.XGMI_LINK_GBPS_ASSUMED * 1e3) + bench.XCHG_LATENCY_US_ASSUMED


def emulate(L, n, tol, pd):
    rd, it_s, it_r = C.c_double(0), C.c_int(0), C.c_int(0)
    us, xd, mm = (C.c_double * 8)(), (C.c_longlong * 3)(), (C.c_int * 2)()
    rc = L.dkmc_xtb_emulate_slabs(n, 16, tol, n // 2, 0, C.byref(rd), C.byref(it_s), C.byref(it_r), us, xd, mm)
    if rc != 0:
        err = L.dkmc_last_error().decode(); L.dkmc_clear_error()
        raise RuntimeError("dkmc_xtb_emulate_slabs(%d) failed: %s" % (n, err[:200]))
    ex, hd, nm = C.c_int(0), C.c_longlong(0), C.c_double(0)
    L.dkmc_xtb_slab_last(C.byref(ex), C.byref(hd), C.byref(nm))
    kern = sum(us[i] for i in range(8)) + 2 * pd * nm.value                  # the N products are timed apart from the eight classes
    x1, x2, x3 = pair_us(xd[0], n), (0.0 if n == 1 else 25.0), pair_us(xd[2], n)
    xh = 2 * pd * pair_us(hd.value, n, peers=2) if n > 1 else 0.0           # halo exchanges: a lateral slab has (at most) two neighbour slabs
    return {"sweeps": it_s.value, "sweeps_one_gpu_reference": it_r.value, "rel_diff_vs_one_gpu": rd.value,
            "kernel_us": {name: round(us[i], 1) for i, name in enumerate(bench.SLAB_CLASSES)}, "nmul_us": round(nm.value, 2),
            "kernels_us_per_sweep": round(kern, 1), "exchanges_per_sweep": ex.value, "halo_doubles_per_exchange": hd.value,
            "doubles_received_per_sweep_exchanges_1_2_3": list(xd), "rows_per_slab_min_max": [mm[0], mm[1]],
            "exchange_us_per_sweep_ASSUMED": round(x1 + x2 + x3 + xh, 1), "sweep_us": round(kern + x1 + x2 + x3 + xh, 1)}


def model(name, steps):
    import torch
    sim = bench.Sim(name, "cuda:0")
    L = sim.L
    pd = L.dkmc_get_x_poly()
    el, done = sim.run(steps, 1)
    step_ms = el / done * 1e3
    iters = sim.cnt["cg_iters_X"] / max(done, 1)
    tol = sim.p.cg_tol
    out = {"workload": name, "sites": int(sim.dev.N), "cg_tol": tol, "x_poly": pd, "single_gpu_ms_per_step": round(step_ms, 1),
           "single_gpu_sweeps_per_step": iters, "by_switch": {}}
    try:
        for sw in (0, 1):
            L.dkmc_set_x_slab_poly(sw)
            rows = {n: emulate(L, n, tol, pd if sw else 0) for n in (1, 2, 4, 8)}
            out["by_switch"]["on" if sw else "off"] = rows
    finally:
        L.dkmc_set_x_slab_poly(0)
    # step_N = outside + sweeps per step x sweep_N; the single-GPU step runs the preconditioned loop, so its sweeps price the "on" rows; the plain
    # loop's sweeps per step are scaled by the emulated ratio plain / preconditioned at N = 1
    on, off = out["by_switch"]["on"], out["by_switch"]["off"]
    outside = step_ms - iters * on[1]["sweep_us"] * 1e-3
    out["outside_the_sweeps_ms"] = round(outside, 1)
    for key, rows in (("on", on), ("off", off)):
        scale = rows[1]["sweeps"] / max(on[1]["sweeps"], 1)
        t1 = outside + iters * scale * rows[1]["sweep_us"] * 1e-3
        for n, r in rows.items():
            tn = outside + iters * scale * (r["sweeps"] / max(rows[1]["sweeps"], 1)) * r["sweep_us"] * 1e-3
            r["modelled_ms_per_step_ASSUMED_exchanges"] = round(tn, 1)
            r["modelled_speedup_vs_same_switch_N1_ASSUMED_exchanges"] = round(t1 / tn, 2)
            r["modelled_speedup_vs_one_gpu_default_ASSUMED_exchanges"] = round(step_ms / tn, 2)
    sim.close()
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="tile:10,7.5nm")
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slab_poly_model.json"))
    args = ap.parse_args()
    t0 = time.time()
    res = {"what": "slab-distributed block-CG with (dkmc_set_x_slab_poly(1)) and without the split polynomial preconditioner: N virtual ranks on ONE "
                   "GPU (dkmc_xtb_emulate_slabs), sweeps to the default tolerance from a zero start, kernel times of the middle rank (each kernel "
                   "bracketed by events, host-synchronised), exchange payloads counted by the solver",
           "ASSUMED": "exchange durations are NOT measured: every all-to-all-v = payload / (%g GB/s per link and direction) + %g us (halo exchanges: "
                      "payload over two links), the Gram all-gather 25 us (bench.py's constants); nothing here ran on more than one GPU"
                      % (bench.XGMI_LINK_GBPS_ASSUMED, bench.XCHG_LATENCY_US_ASSUMED),
           "runs": [model(w, args.steps) for w in args.workloads.split(",")]}
    res["wall_s"] = round(time.time() - t0, 1)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    for r in res["runs"]:
        print(r["workload"], "one GPU %.1f ms/step, %.1f sweeps" % (r["single_gpu_ms_per_step"], r["single_gpu_sweeps_per_step"]))
        for key in ("off", "on"):
            for n, x in r["by_switch"][key].items():
                print("  %-3s N=%d sweeps %4d (ref %4d) sweep %8.1f us, %2d exchanges, speed-up %.2f (ASSUMED exchanges)"
                      % (key, n, x["sweeps"], x["sweeps_one_gpu_reference"], x["sweep_us"], x["exchanges_per_sweep"],
                         x["modelled_speedup_vs_one_gpu_default_ASSUMED_exchanges"]))


if __name__ == "__main__":
    main()
