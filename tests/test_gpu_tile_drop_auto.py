"""Auto mode of the live view (dkmc_set_x_tile_drop_auto, on by default; csrc/xt_live.h: xtl_drop_rule, csrc/xtb.hip: xtb_cg): below the measured size
gate nothing changes, bit for bit; with the gate forced down (dkmc_set_x_tile_drop_auto_subblocks) the warm-started solves run their sweeps on the live
tiles at 1e-10 and the cold one does not; an explicit threshold keeps its meaning; the loops that ignore dkmc_set_x_tile_drop ignore auto mode too; and
after a solve on the live view the four dkmc_stats fields that price a sampled tile launch carry the live view's counts.  tile:3 (84 591 sites,
16 242 stored sub-blocks) and the 2.5 nm device; every case restores threshold 0, auto 1 and the measured gate."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_loop_profile import block_plan, samples
from test_gpu_parity import Vd, _fresh_device, get, hip  # noqa: F401
from test_gpu_tile_f32 import _workload

pytestmark = pytest.mark.gpu
THETA = 1e-10
REL_BOUND = 1.97e-7                    # 10 x the measured distance of two admissible solutions: the bound of tests/test_gpu_tile_drop.py
FIELDS = ("log", "m", "power", "pot")


def _info(L):
    from devicekmc_amd.lib import check
    info = (C.c_longlong * 8)(); ms = (C.c_double * 2)()
    check(L.dkmc_get_x_tile_live_info(info, ms))
    return list(info)


def _restore(L):
    L.dkmc_set_x_tile_drop(0.0); L.dkmc_set_x_tile_drop_auto(1); L.dkmc_set_x_tile_drop_auto_subblocks(0)


def _supersteps(structure, p, hip, n, auto, gate, theta=0.0, warm=1, profile_step=-1):
    """n coupled supersteps on a fresh device with the three switches set; per step the results, the report and the stats"""
    host, L = hip
    L.dkmc_set_x_tile_drop(theta); L.dkmc_set_x_tile_drop_auto(auto); L.dkmc_set_x_tile_drop_auto_subblocks(gate)
    dev, sim, gb, _ = _fresh_device(structure, p, hip, warm=warm)
    rec = []
    for k in range(n):
        dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, k)
        _, dt = sim.executeKMCStep(gb, dev, want_log=True)
        L.dkmc_set_profiling(1 if k == profile_step else 0)
        dev.updatePower(gb, p, Vd)
        L.dkmc_set_profiling(0)
        st = host.get_stats()
        rec.append(dict(log=np.array(sim.last_event_log).copy(), dt=dt, iters=st["cg_iters_X"], rr=st["cg_rr_X"], im=dev.imacro, power=get(gb, "site_power").copy(),
                        m=get(gb, "atom_virtual_potentials").copy(), pot=get(gb, "site_potential_charge").copy(), info=_info(L), used=L.dkmc_get_x_tile_drop_used(),
                        f64_rounds=st["x_tile_f64_rounds"], st=dict(st)))
    return rec, (dev, sim, gb)


def _same_bits(a, b):
    for k, (x, y) in enumerate(zip(a, b)):
        assert x["iters"] == y["iters"] and x["rr"] == y["rr"] and x["im"] == y["im"] and x["dt"] == y["dt"], (k, x["iters"], y["iters"], x["rr"], y["rr"])
        for f in FIELDS:
            assert np.array_equal(x[f], y[f]), (k, f)


@pytest.fixture(scope="module")
def tile3(cell_2p5, dev_7p5):
    structure, p = _workload("tile:3", cell_2p5, dev_7p5)
    p.solve_heating_global = True
    return structure, p


@pytest.fixture(scope="module")
def auto_off_tile3(tile3, hip):
    """three coupled supersteps of tile:3 with auto mode off and no threshold: the full view.  Computed once, shared, left unchanged."""
    try:
        rec, _ = _supersteps(tile3[0], tile3[1], hip, 3, 0, 0)
    finally:
        _restore(hip[1])
    return rec


@pytest.fixture(scope="module")
def forced_tile3(tile3, hip):
    """the same three supersteps with the fresh defaults and the gate forced to one sub-block, then one more with auto mode off"""
    host, L = hip
    structure, p = tile3
    try:
        rec, (dev, sim, gb) = _supersteps(structure, p, hip, 3, 1, 1)
        L.dkmc_set_x_tile_drop_auto(0)
        dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, 3)
        sim.executeKMCStep(gb, dev, want_log=True)
        dev.updatePower(gb, p, Vd)
        after = dict(st=dict(host.get_stats()), info=_info(L), used=L.dkmc_get_x_tile_drop_used())
    finally:
        _restore(L)
    return rec, after


def test_below_the_gate_nothing_changes(tile3, auto_off_tile3, hip):
    """tile:3 lies below the measured gate: the fresh defaults give what auto mode off gives, bit for bit, on the full view."""
    host, L = hip
    assert L.dkmc_get_x_tile_drop() == 0.0 and L.dkmc_get_x_tile_drop_auto() == 1
    try:
        rec, _ = _supersteps(tile3[0], tile3[1], hip, 3, 1, 0)
    finally:
        _restore(L)
    assert L.dkmc_xtl_drop_rule(rec[0]["st"]["xt_subblocks"]) == 0.0
    _same_bits(auto_off_tile3, rec)
    for k, (x, y) in enumerate(zip(auto_off_tile3, rec)):
        assert x["used"] == 0.0 and y["used"] == 0.0 and x["info"][0] == 0 and y["info"][0] == 0, (k, y["used"], y["info"])


def test_gate_forced_warm_steps_run_the_live_view(tile3, auto_off_tile3, forced_tile3):
    """Gate at one sub-block: step 0 has no previous solution and runs the full view, steps 1 and 2 run the live view at 1e-10 without a re-entry
    round; same events as auto mode off, every true residual within the stop test, I_macro and site_power within the bound of test_gpu_tile_drop.py."""
    p = tile3[1]
    rec, _ = forced_tile3
    worst = 0.0
    for k, (x, y) in enumerate(zip(auto_off_tile3, rec)):
        di = abs(y["im"] / x["im"] - 1); dp = np.abs(y["power"] - x["power"]).max() / np.abs(x["power"]).max()
        worst = max(worst, di, dp)
        print("tile:3 step %d: used %.1e, sweeps %d / %d, f64 rounds %d, true residual %.3e / %.3e, info %s, rel dI_macro %.3e, rel dpower %.3e"
              % (k, y["used"], x["iters"], y["iters"], y["f64_rounds"], np.sqrt(x["rr"]), np.sqrt(y["rr"]), y["info"], di, dp))
    assert rec[0]["used"] == 0.0 and rec[0]["info"][0] == 0, (rec[0]["used"], rec[0]["info"])
    _same_bits(auto_off_tile3[:1], rec[:1])                                   # the cold step is the full view's
    for k in (1, 2):
        y = rec[k]
        assert y["used"] == THETA and y["info"][0] == 1 and y["info"][2] < y["info"][1], (k, y["used"], y["info"])
        assert y["f64_rounds"] == 0, (k, y["f64_rounds"])
    for k, (x, y) in enumerate(zip(auto_off_tile3, rec)):
        assert np.array_equal(x["log"], y["log"]) and x["dt"] == y["dt"], k
        assert 0 <= y["rr"] <= p.cg_tol ** 2 and 0 <= x["rr"] <= p.cg_tol ** 2, (k, x["rr"], y["rr"])
    assert worst <= REL_BOUND, worst


def test_stats_describe_the_view_the_sweeps_streamed(auto_off_tile3, forced_tile3):
    """After a live-view solve xt_local_subblocks, spmv_tiles, xt_items and xt_records are the live view's (the events are those of the auto-off run, so
    its stats of the same step describe the same stored X); xt_subblocks stays the stored count; the next full-view solve reports the stored ones again."""
    rec, after = forced_tile3
    for k in (1, 2):
        st, info, full = rec[k]["st"], rec[k]["info"], auto_off_tile3[k]["st"]
        assert st["xt_local_subblocks"] == info[4] and st["spmv_tiles"] == info[2] and st["xt_subblocks"] == info[3], (k, st, info)
        assert st["xt_subblocks"] == full["xt_subblocks"] == full["xt_local_subblocks"] and info[1] == full["spmv_tiles"], (k, info, full)
        assert st["spmv_tile_entries"] == full["spmv_tile_entries"] and st["X_nnz"] == full["X_nnz"]
        assert 0 < st["xt_local_subblocks"] < full["xt_local_subblocks"] and 0 < st["spmv_tiles"] < full["spmv_tiles"]
        assert st["xt_items"] > 0 and st["xt_items"] % 4 == 0 and st["xt_records"] == st["xt_items"] // 4, (k, st["xt_items"], st["xt_records"])
        assert st["xt_items"] <= full["xt_items"] and st["xt_records"] <= full["xt_records"] and full["xt_records"] == full["xt_items"] // 4
    for st, info in ((rec[0]["st"], rec[0]["info"]), (after["st"], after["info"])):
        assert info[0] == 0 and st["xt_local_subblocks"] == st["xt_subblocks"] > 0 and st["xt_records"] == st["xt_items"] // 4, (st, info)
    assert after["used"] == 0.0
    assert rec[0]["st"]["spmv_tiles"] == auto_off_tile3[0]["st"]["spmv_tiles"] and rec[0]["st"]["xt_items"] == auto_off_tile3[0]["st"]["xt_items"]


def test_precedence_of_the_explicit_threshold(tile3, auto_off_tile3, hip):
    """An explicit threshold applies as it is, from the cold step on; auto mode off and no threshold: the full view at any gate."""
    host, L = hip
    try:
        a, _ = _supersteps(tile3[0], tile3[1], hip, 2, 1, 1, theta=1e-12)
        b, _ = _supersteps(tile3[0], tile3[1], hip, 2, 0, 1)
    finally:
        _restore(L)
    for k, y in enumerate(a):
        assert y["used"] == 1e-12 and y["info"][0] == 1, (k, y["used"], y["info"])
        assert 0 <= y["rr"] <= tile3[1].cg_tol ** 2
    assert all(y["used"] == 0.0 and y["info"][0] == 0 for y in b)
    _same_bits(auto_off_tile3[:2], b)


@pytest.mark.parametrize("how", ["x_block(1)", "x_poly(0)", "cg_tol(1e-10)", "warm_start(0)"])
def test_loops_that_ignore_the_switch(cell_2p5, hip, how):
    """The single-vector loop, the loop without preconditioner, a tolerance below the fp32 image's, and zero starts: with the gate forced the solves run
    the full view and give what auto mode off gives, bit for bit."""
    from devicekmc_amd import params as pm
    host, L = hip
    p = pm.KMCParameters(); p.solve_heating_global = True
    d0, auto0 = L.dkmc_get_x_poly(), L.dkmc_get_x_poly_auto()
    warm = 1
    try:
        if how == "x_block(1)":
            L.dkmc_set_x_block(1)
        elif how == "x_poly(0)":
            L.dkmc_set_x_poly(0)
        elif how == "cg_tol(1e-10)":
            p.cg_tol = 1e-10
        else:
            warm = 0
        a, _ = _supersteps(cell_2p5, p, hip, 2, 0, 1, warm=warm)
        b, _ = _supersteps(cell_2p5, p, hip, 2, 1, 1, warm=warm)
    finally:
        _restore(L); L.dkmc_set_current_warm_start(1); L.dkmc_set_x_block(16); L.dkmc_set_x_poly(d0); L.dkmc_set_x_poly_auto(auto0)
    for y in a + b:
        assert y["used"] == 0.0 and y["info"][0] == 0, (how, y["used"], y["info"])
    _same_bits(a, b)


def test_sample_counts_of_the_block_loop_hold_with_the_gate_forced(cell_2p5, hip):
    """The one-GPU block-loop case of test_gpu_loop_profile.py (no preconditioner, zero starts) with the gate forced: the same counts."""
    import test_gpu_loop_profile as lp
    host, L = hip
    d0, auto0 = L.dkmc_get_x_poly(), L.dkmc_get_x_poly_auto()
    try:
        L.dkmc_set_x_tile_drop_auto_subblocks(1)
        lp.test_sampled_profile_follows_the_plan_and_changes_nothing(cell_2p5, hip, "block")
        assert L.dkmc_get_x_tile_drop_used() == 0.0
    finally:
        _restore(L); L.dkmc_set_x_poly(d0); L.dkmc_set_x_poly_auto(auto0)      # (that case leaves the degree pinned)


def test_sample_counts_with_the_view_on(tile3, forced_tile3, hip):
    """tile:3, gate forced, profiling on during the third solve (sweeps on the live view): the sampled launches are those the batch plan gives for the
    hint the second solve left and the sweeps the third took, and profiling changes nothing the solve computes."""
    host, L = hip
    ref, _ = forced_tile3
    try:
        rec, _ = _supersteps(tile3[0], tile3[1], hip, 3, 1, 1, profile_step=2)
    finally:
        _restore(L)
    _same_bits(ref, rec)
    y = rec[2]
    assert y["used"] == THETA and y["info"][0] == 1 and y["f64_rounds"] == 0 and rec[1]["f64_rounds"] == 0
    want = samples(*block_plan(rec[1]["iters"]), y["iters"])
    print("tile:3 view on: hint", rec[1]["iters"], "sweeps", y["iters"], "samples", want, "long", y["st"]["spmv_long_launches"], "short", y["st"]["spmv_short_launches"])
    assert want > 0 and y["st"]["spmv_long_launches"] == want and y["st"]["spmv_short_launches"] == want
    assert y["st"]["spmv_long_ms"] > 0 and y["st"]["spmv_short_ms"] > 0
