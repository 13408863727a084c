#!/usr/bin/env python3
"""The block-CG's tile x panel kernel ALONE on three views of the same resident X: the full fp32 image, the live view of dkmc_set_x_tile_drop with whole
tiles (dkmc_set_x_tile_drop_unit(0)) and with sub-blocks (unit 1).  One process and one solve per workload; then `rounds` rounds, each timing the full
image and, for theta in 1e-10 and 1e-12, the unit-0 and the unit-1 view one after the other (dkmc_xtb_time_apply_stored with stored_bytes 4 / -4: the
view is built afresh with the solve's scaling, every timing the mean of `reps` back-to-back launches).  One JSON line per workload in
<out-dir>/x_tile_drop_unit_apply_<workload>.jsonl: per view the timings [us per launch], their median and spread (max - min), the streamed sub-blocks,
ns per streamed sub-block and the live tiles.  The reference point of a unit-1 view is the unit-0 view of the same theta; a difference counts when it
exceeds 3 x the spread of that reference over its repeats.  Where a view does not exist (fewer than 1 / 64 of the sub-blocks would go: error 13) the
record says so and carries no timing for it.
usage: python tools/time_tile_drop_unit.py [tile:10 tile:5 7.5nm] [--rounds 4] [--reps 5] [--width 16] [--out-dir profiles]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THETAS = (1e-10, 1e-12)


def child(name, rounds, reps, width, out_dir):
    import numpy as np
    import bench
    from devicekmc_amd.lib import DeviceKMCError, check
    sim = bench.Sim(name, "cuda:0")
    L = sim.L
    L.dkmc_set_x_tile_f32(1); L.dkmc_set_x_tile_drop(0.0); L.dkmc_set_x_tile_drop_unit(0)
    sim.step(False)
    st = sim.host.get_stats()
    nt, nsub = C.c_longlong(0), C.c_longlong(0)
    check(L.dkmc_xt_get_tiles(C.byref(nt), C.byref(nsub), None, None))
    tiles = np.zeros((nt.value, 4), dtype=np.int32)
    check(L.dkmc_xt_get_tiles(None, None, tiles.ctypes.data, None))
    popc = np.array([bin(i).count("1") for i in range(256)])
    views = {"full": dict(theta=0.0, unit=None, subblocks=int(nsub.value), tiles=int(nt.value), us=[])}
    for theta in THETAS:
        masks = np.zeros(nt.value, dtype=np.int32)
        check(L.dkmc_xt_get_live_masks(theta, masks.ctypes.data))
        live = masks != 0
        views["%g/u0" % theta] = dict(theta=theta, unit=0, subblocks=int(popc[tiles[live, 2] & 0xff].sum()), tiles=int(live.sum()), us=[])
        views["%g/u1" % theta] = dict(theta=theta, unit=1, subblocks=int(popc[masks & 0xff].sum()), tiles=int(live.sum()),
                                      full_tiles=int((masks == 0xff).sum()), us=[])
    us = C.c_double(0)
    try:
        for _ in range(rounds):
            for v in views.values():
                L.dkmc_set_x_tile_drop(v["theta"]); L.dkmc_set_x_tile_drop_unit(v["unit"] or 0)
                try:
                    check(L.dkmc_xtb_time_apply_stored(width, 4 if v["unit"] is None else -4, reps, C.byref(us)))
                    v["us"].append(round(us.value, 1))
                except DeviceKMCError as ex:      # error 13: no live view at this threshold and unit (too little to drop): the sweeps stream the full image
                    v["no_view"] = str(ex).split(":")[0]      # "devicekmc_hip error 13" (the text behind it names a source line)
    finally:
        L.dkmc_set_x_tile_drop(0.0); L.dkmc_set_x_tile_drop_unit(0)
    for v in views.values():
        if not v["us"]:
            continue
        v["median_us"] = round(float(np.median(v["us"])), 2); v["spread_us"] = round(max(v["us"]) - min(v["us"]), 1)
        v["ns_per_subblock"] = round(1e3 * v["median_us"] / v["subblocks"], 3)
    rec = dict(workload=name, sites=int(sim.s.N), width=width, reps=reps, rounds=rounds, image_bytes=int(st["x_tile_f32_bytes"]), views=views)
    for theta in THETAS:
        a, b = views["%g/u0" % theta], views["%g/u1" % theta]
        if not a["us"] or not b["us"]:
            continue
        gain = round(a["median_us"] - b["median_us"], 1)
        rec["%g" % theta] = dict(unit1_gain_us=gain, unit0_spread_us=a["spread_us"], counts=bool(abs(gain) > 3 * a["spread_us"]),
                                 ratio_unit0_over_unit1=round(a["median_us"] / b["median_us"], 4))
    line = json.dumps(rec)
    with open(os.path.join(out_dir, "x_tile_drop_unit_apply_%s.jsonl" % name.replace(":", "")), "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    sim.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=["tile:10", "tile:5", "7.5nm"])
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int, default=16)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.rounds, a.reps, a.width, a.out_dir)
    os.makedirs(a.out_dir, exist_ok=True)
    for name in a.workloads:      # one process per workload: every workload starts from a fresh library and allocator
        rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--child", name, "--rounds", str(a.rounds), "--reps", str(a.reps), "--width", str(a.width),
                              "--out-dir", a.out_dir])
        if rc:
            print("%s: child ended with %d" % (name, rc), file=sys.stderr)
            sys.exit(1)           # nothing more is started on the GPU after a failure


if __name__ == "__main__":
    main()
