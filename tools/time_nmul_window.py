#!/usr/bin/env python3
"""One N product of the preconditioner's L = p(N) with its panel operands gathered from memory (dkmc_set_x_nmul_window(0): k_xtb_nmulp16) and served
from LDS row windows (1: k_xtb_nmulw), same process, same resident X: `launches` timings of each, alternating, every timing the mean over `reps`
Horner sequences of the degree the solve ran (dkmc_xtb_time_poly); window_us is the default plan.  Further block sizes of the window plan: "block=192,256".
usage: python tools/time_nmul_window.py tile:10 [launches] [reps] [block=B,...]"""
import ctypes as C
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from devicekmc_amd.lib import check  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("block=")]
blocks = [int(b) for a in sys.argv[1:] if a.startswith("block=") for b in a[6:].split(",")]
name = args[0] if len(args) > 0 else "tile:5"
launches = int(args[1]) if len(args) > 1 else 8
reps = int(args[2]) if len(args) > 2 else 4
sim = bench.Sim(name, "cuda:0", cg_tol=1e-3)
sim.step(False)
st = sim.host.get_stats()
degree = int(st["xb_poly_used"])
out = {"workload": name, "sites": int(sim.s.N), "rows": int(st["N_atom"]) + 1, "degree": degree, "reps": reps, "gather_us": [], "window_us": []}
forms = [(0, 0, "gather_us"), (1, 0, "window_us")] + [(1, b, "window_b%d_us" % b) for b in blocks]
for _, _, key in forms:
    out.setdefault(key, [])
try:
    for _ in range(launches):
        for mode, block, key in forms:
            sim.L.dkmc_set_x_nmul_window(mode)
            sim.L.dkmc_debug_set_x_nmul_window(-1, block)
            us = C.c_double(0)
            check(sim.L.dkmc_xtb_time_poly(degree, reps, C.byref(us)))
            out[key].append(round(us.value, 2))
finally:
    sim.L.dkmc_debug_set_x_nmul_window(-1, 0)
    sim.L.dkmc_set_x_nmul_window(2)
med = lambda v: sorted(v)[len(v) // 2]
for _, _, key in forms:
    out[key.replace("_us", "_median_us")] = med(out[key])
out["gather_spread_us"] = round(max(out["gather_us"]) - min(out["gather_us"]), 2)
out["gain_us"] = round(out["gather_median_us"] - out["window_median_us"], 2)
out["gain_exceeds_3x_gather_spread"] = bool(out["gain_us"] > 3 * out["gather_spread_us"])
print(json.dumps(out))
