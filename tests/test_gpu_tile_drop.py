"""Opt-in sweeps on the live tiles only (dkmc_set_x_tile_drop; csrc/xt_live.h, csrc/xtb.hip): the census against the host, the tile x panel product on
the compact image against the host, coupled supersteps with the switch at 0 and at 1e-10, the safety net (a failed true-residual check re-enters on
the fp64 store) and the loops that ignore the switch.  The contract is the block loop's: the SOLUTION within the reference's stop test on column 0,
checked in fp64 on the full store at the end of every solve."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import Vd, _fresh_device, get, hip  # noqa: F401
from test_gpu_tile_f32 import PRODUCT_FP64_MEASURED, SOLVE_REL_MEASURED, _test_panel, _workload

pytestmark = pytest.mark.gpu


def _scaled_residual(rp, ci, data, m_scaled, G0, loop_G, Vd=Vd):
    """||S (X m - b)||_2 with S = diag(X)^-1/2: the quantity the stop test bounds (the CSR residual helper of test_gpu_block_cg.py, copied)."""
    import scipy.sparse as sp
    n = len(rp) - 1
    X = sp.csr_matrix((data, ci, rp), shape=(n, n))
    b = np.zeros(n); b[0] = -loop_G * Vd; b[1] = loop_G * Vd
    s = 1.0 / np.sqrt(X.diagonal())
    return float(np.linalg.norm(s * (X @ (m_scaled[:n] / G0) - b)))


def _info(L):
    from devicekmc_amd.lib import check
    info = (C.c_longlong * 8)(); ms = (C.c_double * 2)()
    check(L.dkmc_get_x_tile_live_info(info, ms))
    return list(info)


def test_default_and_clamping(hip):
    host, L = hip
    try:
        assert L.dkmc_get_x_tile_drop() == 0.0                             # a fresh library, and what every test leaves behind
        for v in (-1.0, float("nan"), 0.0):
            L.dkmc_set_x_tile_drop(1e-10); L.dkmc_set_x_tile_drop(v)
            assert L.dkmc_get_x_tile_drop() == 0.0, v
        L.dkmc_set_x_tile_drop(1e-10)
        assert L.dkmc_get_x_tile_drop() == 1e-10
        L.dkmc_set_x_tile_drop(1.0)
        assert L.dkmc_get_x_tile_drop() == 1e-4
    finally:
        L.dkmc_set_x_tile_drop(0.0)


@pytest.fixture(scope="module")
def solved_2p5(cell_2p5, hip):
    """The 2.5nm device after one current solve with the switch off, and the host's view of its tunnelling block: tile list, fp64 values, the solve's
    scaling by S rank, the largest scaled magnitude of every stored sub-block and tile.  Computed once, shared, left unchanged."""
    from devicekmc_amd import params as pm
    from devicekmc_amd.lib import check
    host, L = hip
    p = pm.KMCParameters(); p.solve_heating_global = False
    L.dkmc_set_x_tile_drop(0.0); L.dkmc_set_x_tile_f32(1)
    dev, sim, gb, _ = _fresh_device(cell_2p5, p, hip)
    dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, 0); dev.updatePower(gb, p, Vd)
    st = host.get_stats()
    assert st["x_tile_stream"] == 1 and _info(L)[0] == 0
    nt, nsub = C.c_longlong(0), C.c_longlong(0)
    check(L.dkmc_xt_get_tiles(C.byref(nt), C.byref(nsub), None, None))
    tiles = np.zeros((nt.value, 4), dtype=np.int32); tval = np.zeros(nsub.value * 1024)
    check(L.dkmc_xt_get_tiles(None, None, tiles.ctypes.data, tval.ctypes.data))
    ns = st["xt_ns"]
    sS = np.zeros(ns); flags = np.zeros(nt.value, dtype=np.int32)
    check(L.dkmc_xt_get_live(1.0, flags.ctypes.data, sS.ctypes.data))
    assert np.all(sS > 0) and np.all(np.isfinite(sS))
    sSp = np.zeros(256 * ((ns + 255) // 256) + 256); sSp[:ns] = sS
    B = tval.reshape(-1, 32, 32)
    submax = np.zeros(nsub.value); tmax = np.zeros(nt.value)
    for t, (k, w, mask, soff) in enumerate(tiles.astype(np.int64)):
        sl = 0
        for q in range(8):
            if (int(mask) >> q) & 1:
                # the library's order of the two multiplications: (sS_i |v|) sS_j
                submax[soff + sl] = ((sSp[32 * k:32 * k + 32, None] * np.abs(B[soff + sl])) * sSp[None, 256 * w + 32 * q:256 * w + 32 * q + 32]).max()
                sl += 1
        tmax[t] = submax[soff:soff + sl].max()
    return dict(dev=dev, gb=gb, p=p, tiles=tiles.astype(np.int64), tval=tval, B=B, sS=sS, ns=ns, submax=submax, tmax=tmax, theta=float(np.median(tmax)))


def _host_live(s, theta):
    """host flags; which of them sit within 1e-12 relative of theta (their flag is not compared)"""
    return s["tmax"] >= theta, np.abs(s["tmax"] - theta) <= 1e-12 * theta


def test_census_matches_the_host(solved_2p5, hip):
    """theta = the median of the tiles' largest scaled magnitudes: the library's live flags equal the host's for every tile whose largest magnitude is not
    within 1e-12 relative of theta (at most 1 % of the tiles may be left out for that reason), and the report of the next solve carries the host's counts.
    The device holds full and partial tiles."""
    from devicekmc_amd.lib import check
    host, L = hip
    s = solved_2p5; theta = s["theta"]
    masks = s["tiles"][:, 2]
    assert np.any(masks == 0xff) and np.any(masks != 0xff)
    live, near = _host_live(s, theta)
    print("2.5nm: %d tiles, %d sub-blocks, theta (median) %.3e, tile maxima %.3e ... %.3e, within 1e-12 of theta: %d" %
          (len(live), len(s["submax"]), theta, s["tmax"].min(), s["tmax"].max(), near.sum()))
    assert near.sum() <= 0.01 * len(live)
    flags = np.zeros(len(live), dtype=np.int32)
    check(L.dkmc_xt_get_live(theta, flags.ctypes.data, None))
    assert np.array_equal(flags[~near] != 0, live[~near])
    try:
        L.dkmc_set_x_tile_drop(theta)
        s["dev"].updatePower(s["gb"], s["p"], Vd)                            # the same state: the same X and scaling
        info = _info(L)
        st = host.get_stats()
    finally:
        L.dkmc_set_x_tile_drop(0.0)
    nsub_t = np.array([bin(int(m)).count("1") for m in masks])
    lib_live = flags != 0
    assert info[0] == 1, info
    assert info[1] == len(live) and info[3] == len(s["submax"]) == nsub_t.sum()
    assert info[2] == lib_live.sum() and info[4] == nsub_t[lib_live].sum(), info
    assert abs(info[2] - live.sum()) <= near.sum()
    own = (s["submax"] >= theta).sum(); own_near = (np.abs(s["submax"] - theta) <= 1e-12 * theta).sum()
    assert abs(info[5] - own) <= own_near and info[5] <= info[4], (info, own)
    assert info[6] == 4096 * (info[4] + 4) and 0 <= info[7] <= st["cg_iters_X"], (info, st["cg_iters_X"])
    assert st["x_tile_stream"] == 1 and 0 <= st["cg_rr_X"] <= s["p"].cg_tol ** 2


def _host_product(s, live, Q):
    """tile sums of the live tiles, values rounded to float32, accumulated in fp64, both triangles from one stored value"""
    ns_pad = 256 * ((s["ns"] + 255) // 256) + 256
    out = np.zeros((ns_pad, 16)); Qp = np.zeros((ns_pad, 16)); Qp[:s["ns"]] = Q
    for t, (k, w, mask, soff) in enumerate(s["tiles"]):
        if not live[t]:
            continue
        sl = 0
        for q in range(8):
            if (int(mask) >> q) & 1:
                b = s["B"][soff + sl].astype(np.float32).astype(np.float64); sl += 1
                rows = slice(32 * k, 32 * k + 32); cols = slice(256 * w + 32 * q, 256 * w + 32 * q + 32)
                out[rows] += b @ Qp[cols]; out[cols] += b.T @ Qp[rows]
    return out


def test_product_on_the_live_image(solved_2p5, hip):
    """k_xtb_apply<..., float> on the compact image and the live launch view (dkmc_xtb_tile_product(width, -4)) against the host: the float-rounded values
    of the live tiles only, both triangles, accumulated in fp64.  Bound: the one test_gpu_tile_f32.py uses for the full image (4 x the fp64 form's
    measured agreement, scaled by the largest sum).  Widths 16, 8, 4."""
    from devicekmc_amd.lib import check
    host, L = hip
    s = solved_2p5; theta = s["theta"]
    flags = np.zeros(len(s["tmax"]), dtype=np.int32)
    check(L.dkmc_xt_get_live(theta, flags.ctypes.data, None))
    live, near = _host_live(s, theta)
    assert np.array_equal(flags[~near] != 0, live[~near])
    ref = _host_product(s, flags != 0, _test_panel(s["ns"]))
    full = np.zeros((s["ns"], 16))
    try:
        L.dkmc_set_x_tile_drop(theta)
        check(L.dkmc_xtb_tile_product(16, 4, full.ctypes.data))
        for width in (16, 8, 4):
            got = np.zeros((s["ns"], width))
            check(L.dkmc_xtb_tile_product(width, -4, got.ctypes.data))
            big = np.abs(ref[:s["ns"], :width]).max()
            err = np.abs(got - ref[:s["ns"], :width]).max() / big
            print("2.5nm width %d: live image vs host %.3e scaled (largest sum %.3e)" % (width, err, big))
            assert err <= 4 * PRODUCT_FP64_MEASURED["2.5nm"], (width, err)
            assert not np.array_equal(got, full[:, :width])                 # the dead tiles are really left out
    finally:
        L.dkmc_set_x_tile_drop(0.0)


def test_every_tile_dead_gives_exact_zeros(solved_2p5, hip):
    """theta = 1e-4 (the largest the switch keeps): where the host finds every tile dead, a full-view launch followed by the live view's product must give
    tile sums of exactly 0.0 -- the partial arrays hold the full launch's sums in between (the stale-partial trap; dkmc_xtb_tile_product(.., -4) runs
    a full-view launch first, as a solve does).  Where the host finds a live tile at 1e-4 the case does not exist for this device: the library must
    then agree on which tiles those are (the trap itself is covered at the median threshold by test_product_on_the_live_image)."""
    from devicekmc_amd.lib import check
    host, L = hip
    s = solved_2p5
    live, near = _host_live(s, 1e-4)
    print("2.5nm: largest scaled magnitude of a stored entry %.3e; tiles live at 1e-4: %d of %d" % (s["tmax"].max(), live.sum(), len(live)))
    if live.any() or near.any():
        flags = np.zeros(len(live), dtype=np.int32)
        check(L.dkmc_xt_get_live(1e-4, flags.ctypes.data, None))
        assert np.array_equal(flags[~near] != 0, live[~near])
        return
    try:
        L.dkmc_set_x_tile_drop(1e-4)
        full = np.zeros((s["ns"], 16)); got = np.ones((s["ns"], 16))
        check(L.dkmc_xtb_tile_product(16, 8, full.ctypes.data))
        assert np.abs(full).max() > 0
        check(L.dkmc_xtb_tile_product(16, -4, got.ctypes.data))
        assert np.all(got == 0.0)
    finally:
        L.dkmc_set_x_tile_drop(0.0)


def _supersteps(structure, p, hip, theta, n=3, csr=False):
    """n coupled supersteps, warm start on, with the switch at theta"""
    host, L = hip
    L.dkmc_set_x_tile_drop(theta)
    dev, sim, gb, _ = _fresh_device(structure, p, hip, warm=1)
    rec = []
    for k in range(n):
        dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, k)
        sim.executeKMCStep(gb, dev, want_log=True)
        dev.updatePower(gb, p, Vd)
        st = host.get_stats()
        r = dict(log=np.array(sim.last_event_log).copy(), iters=st["cg_iters_X"], rr=st["cg_rr_X"], im=dev.imacro, power=get(gb, "site_power").copy(),
                 m=get(gb, "atom_virtual_potentials").copy(), pot=get(gb, "site_potential_charge").copy(), info=_info(L), f64_rounds=st["x_tile_f64_rounds"],
                 stream=st["x_tile_stream"])
        if csr:
            rp, ci, data = host.get_last_X()
            r["resid"] = _scaled_residual(rp, ci, data, r["m"], p.G0, p.X_loop_G)
            del rp, ci, data
        rec.append(r)
    return rec


def test_solve_contract_tile3(cell_2p5, dev_7p5, hip):
    """tile:3 (57 790 rows), three coupled supersteps, warm start on, theta = 1e-10 against theta = 0 in one process: identical event logs, every solve's
    TRUE scaled residual (host, CSR of the stored X) within the stop test, the compact image streamed with tiles dropped on every step, I_macro and
    site_power within the bound of the fp32-image test (10 x the measured distance of two admissible solutions)."""
    host, L = hip
    structure, p = _workload("tile:3", cell_2p5, dev_7p5)
    p.solve_heating_global = True
    try:
        a = _supersteps(structure, p, hip, 0.0)
        b = _supersteps(structure, p, hip, 1e-10, csr=True)
    finally:
        L.dkmc_set_x_tile_drop(0.0)
    worst = 0.0
    for k, (x, y) in enumerate(zip(a, b)):
        di = abs(y["im"] / x["im"] - 1); dp = np.abs(y["power"] - x["power"]).max() / np.abs(x["power"]).max()
        worst = max(worst, di, dp)
        print("tile:3 step %d: sweeps %d / %d, f64 rounds %d / %d, true residual (library) %.3e / %.3e, (host CSR, theta 1e-10) %.3e, info %s, rel dI_macro %.3e, rel dpower %.3e"
              % (k, x["iters"], y["iters"], x["f64_rounds"], y["f64_rounds"], np.sqrt(x["rr"]), np.sqrt(y["rr"]), y["resid"], y["info"], di, dp))
    for k, (x, y) in enumerate(zip(a, b)):
        assert x["info"][0] == 0 and x["stream"] == 1 and y["stream"] == 1, (k, x["info"])
        assert np.array_equal(x["log"], y["log"]), k
        assert x["rr"] <= p.cg_tol ** 2 and y["rr"] <= p.cg_tol ** 2, (k, x["rr"], y["rr"])
        assert y["resid"] <= p.cg_tol, (k, y["resid"])
        assert y["info"][0] == 1 and y["info"][2] < y["info"][1], (k, y["info"])
    assert worst <= 10 * SOLVE_REL_MEASURED, worst


def test_safety_net_reenters_on_the_fp64_store(cell_2p5, hip):
    """2.5nm from a zero start (dkmc_set_current_warm_start(0)) with theta = 1e-6: the dropped entries act on the whole solution, the true-residual check
    fails, and the solve is re-entered on the full fp64 store and ends within the stop test."""
    from devicekmc_amd import params as pm
    host, L = hip
    p = pm.KMCParameters(); p.solve_heating_global = False
    try:
        L.dkmc_set_x_tile_drop(1e-6)
        dev, sim, gb, _ = _fresh_device(cell_2p5, p, hip, warm=0)
        dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, 0); dev.updatePower(gb, p, Vd)
        st = host.get_stats(); info = _info(L)
        print("2.5nm zero start, theta 1e-6: info %s, sweeps %d, f64 rounds %d, true residual %.3e" % (info, st["cg_iters_X"], st["x_tile_f64_rounds"], np.sqrt(st["cg_rr_X"])))
        rp, ci, data = host.get_last_X()
        assert _scaled_residual(rp, ci, data, get(gb, "atom_virtual_potentials"), p.G0, p.X_loop_G) <= p.cg_tol
        assert 0 <= st["cg_rr_X"] <= p.cg_tol ** 2 and st["xb_fallback"] == 0
        assert info[0] == 1 and st["x_tile_f64_rounds"] >= 1, (info, st["x_tile_f64_rounds"])
    finally:
        L.dkmc_set_x_tile_drop(0.0); L.dkmc_set_current_warm_start(1)


@pytest.mark.parametrize("how", ["x_poly(0)", "x_block(1)", "x_tile_f32(0)"])
def test_loops_that_ignore_the_switch(cell_2p5, hip, how):
    """Preconditioner off, the single-vector loop, the fp64 stream: the report says "not applicable" and the potentials equal the theta = 0 run's bit for bit."""
    from devicekmc_amd import params as pm
    host, L = hip
    p = pm.KMCParameters(); p.solve_heating_global = True
    d0, auto0 = L.dkmc_get_x_poly(), L.dkmc_get_x_poly_auto()
    try:
        if how == "x_poly(0)":
            L.dkmc_set_x_poly(0)
        elif how == "x_block(1)":
            L.dkmc_set_x_block(1)
        else:
            L.dkmc_set_x_tile_f32(0)
        a = _supersteps(cell_2p5, p, hip, 0.0, n=2)
        b = _supersteps(cell_2p5, p, hip, 1e-10, n=2)
    finally:
        L.dkmc_set_x_tile_drop(0.0); L.dkmc_set_x_tile_f32(1); L.dkmc_set_x_block(16); L.dkmc_set_x_poly(d0); L.dkmc_set_x_poly_auto(auto0)
    for x, y in zip(a, b):
        assert y["info"][0] == 0 and x["info"][0] == 0, y["info"]
        assert x["iters"] == y["iters"] and x["rr"] == y["rr"] and x["im"] == y["im"]
        for f in ("log", "m", "power", "pot"):
            assert np.array_equal(x[f], y[f]), f
