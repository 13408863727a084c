#!/usr/bin/env python3
"""The block-CG's tile x panel kernel on the fp64 store and on its fp32 image (dkmc_set_x_tile_f32), same process, same resident X: `launches` timings
of each, alternating, every timing the mean of 5 back-to-back launches (dkmc_xtb_time_apply_stored).
usage: python tools/time_xtb_apply_stored.py tile:10 [width] [launches]"""
import ctypes as C
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from devicekmc_amd.lib import check  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "tile:5"
width = int(sys.argv[2]) if len(sys.argv) > 2 else 16
launches = int(sys.argv[3]) if len(sys.argv) > 3 else 8
sim = bench.Sim(name, "cuda:0", cg_tol=1e-3)
sim.L.dkmc_set_x_tile_f32(1)
sim.step(False)
st = sim.host.get_stats()
nsub = int(st["xt_subblocks"])
out = {"workload": name, "sites": int(sim.s.N), "width": width, "subblocks": nsub, "image_bytes": int(st["x_tile_f32_bytes"]), "fp64_us": [], "fp32_us": []}
for _ in range(launches):
    for stored, key in ((8, "fp64_us"), (4, "fp32_us")):
        us = C.c_double(0)
        check(sim.L.dkmc_xtb_time_apply_stored(width, stored, 5, C.byref(us)))
        out[key].append(round(us.value, 1))
med = lambda v: sorted(v)[len(v) // 2]
out["fp64_median_us"], out["fp32_median_us"] = med(out["fp64_us"]), med(out["fp32_us"])
out["fp64_spread_us"] = round(max(out["fp64_us"]) - min(out["fp64_us"]), 1)
out["gain_us"] = round(out["fp64_median_us"] - out["fp32_median_us"], 1)
out["gain_exceeds_3x_fp64_spread"] = bool(out["gain_us"] > 3 * out["fp64_spread_us"])
out["fp64_tile_GBps"] = round(8192 * nsub / out["fp64_median_us"] / 1e3, 1)
out["fp32_tile_GBps"] = round(4096 * nsub / out["fp32_median_us"] / 1e3, 1)
print(json.dumps(out))
