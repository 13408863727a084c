#!/usr/bin/env python3
"""The degree of the split polynomial preconditioner against the system size, in the headline's own regime (warm-started steady steps): one bench.py
run with the degree forced, one JSON record appended to a file.

usage: python tools/x_poly_by_size.py DEGREE RECORD_FILE [bench.py arguments ...]
       DEGREE = an integer (dkmc_set_x_poly(DEGREE): pins it) or `default` (the library's defaults untouched: the rule where the library has one);
                with `+split` behind it the split form is forced (dkmc_set_x_poly_form(0)), with `+one` the one-polynomial form (1) at the level's own
                degree n(d), with `+one:N` at degree N (dkmc_debug_set_x_poly1_degree), e.g. `default+one:16`
       python tools/x_poly_by_size.py compare REF_DUMP_DIR DUMP_DIR RECORD_FILE     (two --dump-outputs directories of the same steps)
       python tools/x_poly_by_size.py best RECORD_FILE                              (appends the best degree of every measured size)

The record: steps/s, sweeps per step (mean and each), the tile kernel's and the row kernel's time per working launch (HIP events of the timed steps),
and of every timed step the true residual of column 0, whether the solve re-entered on the fp64 store (dkmc_stats.x_tile_f64_rounds), whether the
block loop fell back, and the degree the solve ran (dkmc_stats.xb_poly_used, where the library reports it).  The N product's time per launch is not
in the event profile: it comes from the rocprofv3 kernel traces beside the record file (profiles/README.md)."""
import contextlib
import io
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


class Tee(io.StringIO):
    def write(self, s):
        sys.__stdout__.write(s)
        return super().write(s)


def compare(ref, other, record):
    """Two --dump-outputs directories of the same steps at two degrees: equal event outcome (dt, site_element, site_charge), relative deviations."""
    import numpy as np
    a = {n: np.load(os.path.join(ref, n + ".npy")) for n in ("dt", "I_macro", "site_element", "site_charge", "site_power")}
    b = {n: np.load(os.path.join(other, n + ".npy")) for n in a}
    rec = {"compare": os.path.basename(other.rstrip("/")), "against": os.path.basename(ref.rstrip("/")),
           "same_events": bool(all(np.array_equal(a[n], b[n]) for n in ("dt", "site_element", "site_charge"))),
           "rel_dev_I_macro": float(abs(b["I_macro"][0] / a["I_macro"][0] - 1)),
           "rel_dev_site_power": float(np.abs(b["site_power"] - a["site_power"]).max() / np.abs(a["site_power"]).max())}
    with open(record, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))


def best(record, same_size=0.001):
    """Append one `best_degree` record per measured workload: per degree the median steps/s of its runs; the spread of the size = the largest
    (max - min) / median over the degrees that were run more than once there; the fastest degree, moved to the lower neighbour while that one lies
    within the spread of the fastest.  Workloads whose rows differ by less than `same_size` are ONE size to a rule on the rows: their best degree is the
    one with the largest geometric mean, over those workloads, of steps/s relative to degree 8 (each workload's own result stays in the record)."""
    import statistics
    runs = [r for r in map(json.loads, open(record)) if "steps_per_s" in r and isinstance(r.get("degree"), int) and not r.get("with_live_view")]      # (the lines recorded with the live view on are a record beside the rule, not part of it)
    wls = {}
    for r in runs:
        wls.setdefault(r["workload"], []).append(r)
    info = {}
    for w, rs in wls.items():
        by = {}
        for r in rs:
            by.setdefault(r["degree"], []).append(r["steps_per_s"])
        med = {d: statistics.median(v) for d, v in sorted(by.items())}
        spread = max([(max(v) - min(v)) / statistics.median(v) for v in by.values() if len(v) > 1] or [0.0])
        d = max(med, key=med.get)
        fastest = d
        lower = [x for x in med if x < d]
        while lower and med[max(lower)] >= med[fastest] * (1.0 - spread):
            d = max(lower); lower = [x for x in med if x < d]
        info[w] = dict(rows=rs[0]["rows"], tunnelling_set=rs[0]["tunnelling_set"], med=med, spread=spread, fastest=fastest, own=d)
    out = []
    for w, a in sorted(info.items(), key=lambda kv: kv[1]["rows"]):
        group = [v for v, b in info.items() if abs(b["rows"] - a["rows"]) <= same_size * a["rows"]]
        rec = {"workload": w, "rows": a["rows"], "tunnelling_set": a["tunnelling_set"], "median_steps_per_s_by_degree": {str(d): m for d, m in a["med"].items()},
               "spread": a["spread"], "fastest_degree": a["fastest"], "best_degree": a["own"], "best_degree_of_the_workload": a["own"]}
        if len(group) > 1:
            common = set.intersection(*[set(info[v]["med"]) for v in group])
            gm = {d: math.exp(sum(math.log(info[v]["med"][d] / info[v]["med"][8]) for v in group) / len(group)) for d in common}
            rec["best_degree"] = max(gm, key=gm.get)
            rec["same_size_as"] = [v for v in group if v != w]
            rec["geometric_mean_vs_degree_8"] = {str(d): round(g, 4) for d, g in sorted(gm.items())}
        out.append(rec)
    with open(record, "a") as f:
        for rec in out:
            f.write(json.dumps(rec) + "\n")
            print(json.dumps(rec))


def main():
    if sys.argv[1] == "compare":
        return compare(sys.argv[2], sys.argv[3], sys.argv[4])
    if sys.argv[1] == "best":
        return best(sys.argv[2])
    degree, record = sys.argv[1], sys.argv[2]
    sys.argv = [os.path.join(bench.ROOT, "bench.py")] + sys.argv[3:]
    from devicekmc_amd import host, lib
    L = lib.load()
    degree, _, form = degree.partition("+")
    if degree != "default":
        L.dkmc_set_x_poly(int(degree))
    if form:
        L.dkmc_set_x_poly_form(1 if form.startswith("one") else 0)
        L.dkmc_debug_set_x_poly1_degree(int(form.partition(":")[2] or 0))
    solves = []
    step0 = bench.Sim.step

    def step(self, timed):
        t = step0(self, timed)
        if timed:
            st = host.get_stats()
            solves.append((math.sqrt(max(st["cg_rr_X"], 0.0)), int(st["x_tile_f64_rounds"]), int(st["xb_fallback"]), int(st.get("xb_poly_used", -1)),
                           L.dkmc_get_x_poly_form_used(), L.dkmc_get_x_poly_products()))
        return t
    bench.Sim.step = step
    buf = Tee()
    with contextlib.redirect_stdout(buf):
        bench.main()
    line = json.loads([x for x in buf.getvalue().splitlines() if x.startswith("{")][-1])
    detail = json.load(open(line["detail"])) if line.get("detail") else {}
    roof = line.get("roofline") or {}
    rec = {"workload": line["config"]["workload"], "sites": line["config"]["sites"], "rows": line["config"]["atoms"] + 1, "tunnelling_set": line["per_step"]["tunnelling_set"],
           "degree": degree if degree == "default" else int(degree), "degree_used": sorted(set(s[3] for s in solves)),
           "one_polynomial": sorted(set(s[4] for s in solves)), "n_products_per_sweep": sorted(set(s[5] for s in solves)),
           "steps": line["steps"], "warmup": line["warmup"], "steps_per_s": line["value"], "ms_per_step": line["ms_per_step"],
           "sweeps_per_step": line["per_step"]["cg_iters_X"], "sweeps_each": (detail.get("steady") or {}).get("cg_sweeps_X_each"),
           "k_xtb_apply_us": roof.get("avg_launch_us"), "row_kernel_us": roof.get("row_kernel_us"),
           "true_residual_max": max(s[0] for s in solves), "cg_tol": line["config"]["cg_tol"],
           "true_residual_each": [float("%.3e" % s[0]) for s in solves[:64]], "f64_rounds_each": [s[1] for s in solves[:64]],
           "reentered_steps": sum(1 for s in solves if s[1] > 0), "fallback_steps": sum(1 for s in solves if s[2] > 0)}
    with open(record, "a") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
