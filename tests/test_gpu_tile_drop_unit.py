"""Opt-in sub-block unit of the live view (dkmc_set_x_tile_drop_unit(1); csrc/xt_live.h): the switch, the census's reduced masks against the host, the
tile x panel product on the compact image of the live SUB-BLOCKS against the host, coupled supersteps with unit 1 at 1e-10 against theta = 0, the
safety net, and the settings under which the unit has no effect.  The contract is the one of test_gpu_tile_drop.py: the SOLUTION within the
reference's stop test on column 0, checked in fp64 on the full store at the end of every solve."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import Vd, _fresh_device, get, hip  # noqa: F401
from test_gpu_tile_drop import _info, _scaled_residual, _supersteps, solved_2p5  # noqa: F401
from test_gpu_tile_f32 import PRODUCT_FP64_MEASURED, SOLVE_REL_MEASURED, _test_panel, _workload

pytestmark = pytest.mark.gpu


def _off(L):
    L.dkmc_set_x_tile_drop(0.0); L.dkmc_set_x_tile_drop_unit(0)


def test_switch(hip):
    host, L = hip
    try:
        assert L.dkmc_get_x_tile_drop_unit() == 0                          # a fresh library, and what every test leaves behind
        L.dkmc_set_x_tile_drop_unit(1)
        assert L.dkmc_get_x_tile_drop_unit() == 1
        for v in (2, -1, 7):
            L.dkmc_set_x_tile_drop_unit(1); L.dkmc_set_x_tile_drop_unit(v)
            assert L.dkmc_get_x_tile_drop_unit() == 0, v
    finally:
        _off(L)


def _host_masks(s, theta):
    """per stored tile: the host's mask of the sub-blocks live on their own, and the mask of those within 1e-12 relative of theta (not compared)"""
    live = np.zeros(len(s["tiles"]), dtype=np.int64); near = np.zeros(len(s["tiles"]), dtype=np.int64)
    for t, (k, w, mask, soff) in enumerate(s["tiles"]):
        sl = 0
        for q in range(8):
            if (int(mask) >> q) & 1:
                v = s["submax"][soff + sl]; sl += 1
                if v >= theta:
                    live[t] |= 1 << q
                if abs(v - theta) <= 1e-12 * theta:
                    near[t] |= 1 << q
    return live, near


def _popc(a):
    return np.array([bin(int(m)).count("1") for m in a])


def _theta(s):
    """1e-6 where it leaves a live tile with a dead sub-block on this state, else the median of the tiles' maxima (test_gpu_tile_drop.py)"""
    for theta in (1e-6, s["theta"]):
        live, near = _host_masks(s, theta)
        if np.any((live != 0) & (live != s["tiles"][:, 2])):
            return theta, live, near
    raise AssertionError("no threshold leaves a live tile with a dead sub-block")


def _lib_masks(L, s, theta):
    from devicekmc_amd.lib import check
    masks = np.full(len(s["tiles"]), -1, dtype=np.int32)
    check(L.dkmc_xt_get_live_masks(theta, masks.ctypes.data))
    return masks.astype(np.int64)


def test_census_masks_match_the_host(solved_2p5, hip):
    """2.5nm, theta = 1e-6: the library's unit-1 mask of every stored tile equals stored mask & (largest scaled magnitude of the sub-block >= theta) from
    the host, for every sub-block not within 1e-12 relative of theta (at most 1 % of them); the live flags are mask != 0; a solve with unit 1 streams
    the image of the live sub-blocks (state 1, its size from word [5]) and reports the counts of a unit-0 solve of the same state."""
    from devicekmc_amd.lib import check
    host, L = hip
    s = solved_2p5
    theta, live, near = _theta(s)
    stored = s["tiles"][:, 2]
    partial = (live != 0) & (live != stored)
    print("2.5nm: %d tiles, %d sub-blocks, theta %.3e: host live tiles %d with %d sub-blocks, live on their own %d, live tiles with a dead sub-block %d, "
          "sub-blocks within 1e-12 of theta %d" % (len(stored), len(s["submax"]), theta, (live != 0).sum(), _popc(stored[live != 0]).sum(),
                                                  _popc(live).sum(), partial.sum(), _popc(near).sum()))
    assert partial.any()
    assert _popc(near).sum() <= 0.01 * len(s["submax"])
    masks = _lib_masks(L, s, theta)
    assert np.all((masks & ~stored) == 0)
    assert np.array_equal(masks & ~near, live & ~near)
    flags = np.zeros(len(stored), dtype=np.int32)
    check(L.dkmc_xt_get_live(theta, flags.ctypes.data, None))
    assert np.array_equal(flags != 0, masks != 0)
    try:
        L.dkmc_set_x_tile_drop(theta)
        s["dev"].updatePower(s["gb"], s["p"], Vd)                            # the same state: the same X and scaling
        info0 = _info(L)
        L.dkmc_set_x_tile_drop_unit(1)
        s["dev"].updatePower(s["gb"], s["p"], Vd)
        info1 = _info(L); st = host.get_stats()
    finally:
        _off(L)
    print("2.5nm: report with unit 0 %s, with unit 1 %s" % (info0, info1))
    assert info0[0] == 1 and info1[0] == 1, (info0, info1)
    assert info1[1:6] == info0[1:6], (info0, info1)
    assert info1[2] == (masks != 0).sum() and info1[4] == _popc(stored[masks != 0]).sum() and info1[5] == _popc(masks).sum(), info1
    assert info0[6] == 4096 * (info0[4] + 4) and info1[6] == 4096 * (info1[5] + 4) and info1[5] < info1[4], (info0, info1)
    assert st["x_tile_stream"] == 1 and 0 <= st["cg_rr_X"] <= s["p"].cg_tol ** 2


def _host_product(s, masks, Q):
    """tile sums of the sub-blocks in `masks`, values rounded to float32, accumulated in fp64, both triangles from one stored value"""
    ns_pad = 256 * ((s["ns"] + 255) // 256) + 256
    out = np.zeros((ns_pad, 16)); Qp = np.zeros((ns_pad, 16)); Qp[:s["ns"]] = Q
    for t, (k, w, mask, soff) in enumerate(s["tiles"]):
        sl = 0
        for q in range(8):
            if (int(mask) >> q) & 1:
                if (int(masks[t]) >> q) & 1:
                    b = s["B"][soff + sl].astype(np.float32).astype(np.float64)
                    rows = slice(32 * k, 32 * k + 32); cols = slice(256 * w + 32 * q, 256 * w + 32 * q + 32)
                    out[rows] += b @ Qp[cols]; out[cols] += b.T @ Qp[rows]
                sl += 1
    return out


def test_product_on_the_live_subblocks(solved_2p5, hip):
    """k_xtb_apply<..., float> on the compact image of the live sub-blocks and its launch view (dkmc_xtb_tile_product(width, -4) under unit 1; a full-view
    launch runs first, as in a solve) against the host: the float-rounded values of the live SUB-BLOCKS only, both triangles, accumulated in fp64.
    Bound: the one of the same kernel on the same values (4 x the fp64 form's measured agreement, scaled by the largest sum).  Widths 16, 8, 4.  The
    result differs from the unit-0 product: the dead sub-blocks of the live tiles are really left out."""
    from devicekmc_amd.lib import check
    host, L = hip
    s = solved_2p5
    theta, live, near = _theta(s)
    masks = _lib_masks(L, s, theta)
    assert np.array_equal(masks & ~near, live & ~near)
    assert np.any((masks != 0) & (masks != s["tiles"][:, 2]))
    ref = _host_product(s, masks, _test_panel(s["ns"]))
    try:
        L.dkmc_set_x_tile_drop(theta)
        for width in (16, 8, 4):
            tiles_only = np.zeros((s["ns"], width)); got = np.zeros((s["ns"], width))
            L.dkmc_set_x_tile_drop_unit(0)
            check(L.dkmc_xtb_tile_product(width, -4, tiles_only.ctypes.data))
            L.dkmc_set_x_tile_drop_unit(1)
            check(L.dkmc_xtb_tile_product(width, -4, got.ctypes.data))
            big = np.abs(ref[:s["ns"], :width]).max()
            err = np.abs(got - ref[:s["ns"], :width]).max() / big
            print("2.5nm width %d: image of the live sub-blocks vs host %.3e scaled (largest sum %.3e); largest difference to the unit-0 product %.3e scaled"
                  % (width, err, big, np.abs(got - tiles_only).max() / big))
            assert err <= 4 * PRODUCT_FP64_MEASURED["2.5nm"], (width, err)
            assert not np.array_equal(got, tiles_only)
    finally:
        _off(L)


def test_timing_aid_on_the_live_view(solved_2p5, hip):
    """dkmc_xtb_time_apply_stored(width, -4): one launch on the live view at the current threshold, in both units; error 13 where there is no such view."""
    from devicekmc_amd.lib import DeviceKMCError, check
    host, L = hip
    theta, _, _ = _theta(solved_2p5)
    us = C.c_double(-1.0)
    try:
        with pytest.raises(DeviceKMCError, match="error 13"):
            check(L.dkmc_xtb_time_apply_stored(16, -4, 1, C.byref(us)))      # theta = 0: no view
        L.dkmc_set_x_tile_drop(theta)
        for unit in (0, 1):
            L.dkmc_set_x_tile_drop_unit(unit); us.value = -1.0
            check(L.dkmc_xtb_time_apply_stored(16, -4, 1, C.byref(us)))
            assert us.value > 0.0, unit
    finally:
        _off(L)


def test_solve_contract_tile3(cell_2p5, dev_7p5, hip):
    """tile:3, three coupled supersteps, warm start on, unit 1 at theta = 1e-10 against theta = 0 in one process: identical event logs, every solve's
    residual within the stop test (the library's, and the host's on the CSR of the stored X), the image of the live sub-blocks streamed on every step
    with fewer sub-blocks than the live tiles hold, I_macro and site_power within 10 x the measured distance of two admissible solutions."""
    host, L = hip
    structure, p = _workload("tile:3", cell_2p5, dev_7p5)
    p.solve_heating_global = True
    try:
        a = _supersteps(structure, p, hip, 0.0)
        L.dkmc_set_x_tile_drop_unit(1)
        b = _supersteps(structure, p, hip, 1e-10, csr=True)
    finally:
        _off(L)
    worst = 0.0
    for k, (x, y) in enumerate(zip(a, b)):
        di = abs(y["im"] / x["im"] - 1); dp = np.abs(y["power"] - x["power"]).max() / np.abs(x["power"]).max()
        worst = max(worst, di, dp)
        print("tile:3 step %d: sweeps %d / %d, f64 rounds %d / %d, true residual (library) %.3e / %.3e, (host CSR, unit 1 at 1e-10) %.3e, info %s, rel dI_macro %.3e, rel dpower %.3e"
              % (k, x["iters"], y["iters"], x["f64_rounds"], y["f64_rounds"], np.sqrt(x["rr"]), np.sqrt(y["rr"]), y["resid"], y["info"], di, dp))
    for k, (x, y) in enumerate(zip(a, b)):
        assert x["info"][0] == 0 and x["stream"] == 1 and y["stream"] == 1, (k, x["info"])
        assert np.array_equal(x["log"], y["log"]), k
        assert x["rr"] <= p.cg_tol ** 2 and y["rr"] <= p.cg_tol ** 2, (k, x["rr"], y["rr"])
        assert y["resid"] <= p.cg_tol, (k, y["resid"])
        assert y["info"][0] == 1 and y["info"][5] < y["info"][4], (k, y["info"])
        assert y["info"][6] == 4096 * (y["info"][5] + 4), (k, y["info"])
    assert worst <= 10 * SOLVE_REL_MEASURED, worst


def test_safety_net_reenters_on_the_fp64_store(cell_2p5, hip):
    """2.5nm from a zero start with unit 1 at theta = 1e-6: the dropped entries act on the whole solution, the true-residual check fails, and the solve is
    re-entered on the full fp64 store and ends within the stop test."""
    from devicekmc_amd import params as pm
    host, L = hip
    p = pm.KMCParameters(); p.solve_heating_global = False
    try:
        L.dkmc_set_x_tile_drop(1e-6); L.dkmc_set_x_tile_drop_unit(1)
        dev, sim, gb, _ = _fresh_device(cell_2p5, p, hip, warm=0)
        dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, 0); dev.updatePower(gb, p, Vd)
        st = host.get_stats(); info = _info(L)
        print("2.5nm zero start, unit 1 at 1e-6: info %s, sweeps %d, f64 rounds %d, true residual %.3e" % (info, st["cg_iters_X"], st["x_tile_f64_rounds"], np.sqrt(st["cg_rr_X"])))
        rp, ci, data = host.get_last_X()
        assert _scaled_residual(rp, ci, data, get(gb, "atom_virtual_potentials"), p.G0, p.X_loop_G) <= p.cg_tol
        assert 0 <= st["cg_rr_X"] <= p.cg_tol ** 2 and st["xb_fallback"] == 0
        assert info[0] == 1 and info[6] == 4096 * (info[5] + 4) and st["x_tile_f64_rounds"] >= 1, (info, st["x_tile_f64_rounds"])
    finally:
        _off(L); L.dkmc_set_current_warm_start(1)


def _same_bits(a, b):
    for x, y in zip(a, b):
        assert x["iters"] == y["iters"] and x["rr"] == y["rr"] and x["im"] == y["im"]
        for f in ("log", "m", "power", "pot"):
            assert np.array_equal(x[f], y[f]), f


def test_unit_without_effect(cell_2p5, hip):
    """Unit 1 with theta = 0, and unit 1 at 1e-10 with the preconditioner off: the report says "off or not applicable" and potentials, power, event log,
    sweeps and the true residual equal the unit-0, theta = 0 run's bit for bit."""
    from devicekmc_amd import params as pm
    host, L = hip
    p = pm.KMCParameters(); p.solve_heating_global = True
    d0, auto0 = L.dkmc_get_x_poly(), L.dkmc_get_x_poly_auto()
    try:
        a = _supersteps(cell_2p5, p, hip, 0.0, n=2)
        L.dkmc_set_x_tile_drop_unit(1)
        b = _supersteps(cell_2p5, p, hip, 0.0, n=2)
        L.dkmc_set_x_tile_drop_unit(0); L.dkmc_set_x_poly(0)
        c = _supersteps(cell_2p5, p, hip, 0.0, n=2)
        L.dkmc_set_x_tile_drop_unit(1)
        d = _supersteps(cell_2p5, p, hip, 1e-10, n=2)
    finally:
        _off(L); L.dkmc_set_x_poly(d0); L.dkmc_set_x_poly_auto(auto0)
    for r in a + b + c + d:
        assert r["info"][0] == 0, r["info"]
    _same_bits(a, b)
    _same_bits(c, d)
