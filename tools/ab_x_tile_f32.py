#!/usr/bin/env python3
"""f32 tiles on / off (dkmc_set_x_tile_f32): the same six supersteps (same seed) with the switch at 0 and at 1 -- block-CG sweeps per step, seconds,
whether the event sequences (dt trace) are identical, max relative |delta I_macro|, and the true residual of column 0 of every solve both ways.
usage: python tools/ab_x_tile_f32.py [workload ...]   (default: 7.5nm tile:10)"""
import json
import math
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

for wl in sys.argv[1:] or ["7.5nm", "tile:10"]:
    res = {}
    for mode in (0, 1):
        sim = bench.Sim(wl, "cuda:0")
        sim.L.dkmc_set_x_tile_f32(mode)
        resid, stream, f64_rounds = [], [], []
        for k in range(6):
            sim.step(True)
            st = sim.host.get_stats()
            resid.append(math.sqrt(max(st["cg_rr_X"], 0.0))); stream.append(int(st["x_tile_stream"])); f64_rounds.append(int(st["x_tile_f64_rounds"]))
        res[mode] = {"sweeps": [n for _, n in sim.step_log], "seconds": [round(t, 4) for t, _ in sim.step_log], "trace": [(float(a), float(b)) for a, b, _ in sim.trace],
                     "true_residual": resid, "stream": stream, "f64_rounds": f64_rounds}
        sim.L.dkmc_set_x_tile_f32(1)
        del sim
    a, b = res[0], res[1]
    print(json.dumps({"workload": wl, "sweeps_f64": a["sweeps"], "sweeps_f32": b["sweeps"], "s_f64": round(sum(a["seconds"][2:]), 4), "s_f32": round(sum(b["seconds"][2:]), 4),
                      "same_dt_sequence": all(x[0] == y[0] for x, y in zip(a["trace"], b["trace"])),
                      "max_rel_dev_I_macro": max(abs(x[1] - y[1]) / max(abs(x[1]), 1e-300) for x, y in zip(a["trace"], b["trace"])),
                      "true_residual_f64": a["true_residual"], "true_residual_f32": b["true_residual"], "stream_f32": b["stream"],
                      "f64_rounds_f64": a["f64_rounds"], "f64_rounds_f32": b["f64_rounds"]}), flush=True)
