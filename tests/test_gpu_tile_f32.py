"""The fp32 image of the tile values inside the sweeps of the preconditioned block-CG (dkmc_set_x_tile_f32; csrc/xtb.hip, csrc/xt.hip): the tile x panel
product on the image against the host, coupled supersteps with the switch at 0 and 1, the gate that keeps tight tolerances and every other loop on the
fp64 store bit for bit, and the re-entry on the fp64 store after a failed true-residual check.  The contract is the block loop's: the SOLUTION within
the reference's stop test on column 0 (checked in fp64 at the end of every solve), not the iterate sequence."""
import ctypes as C

import numpy as np
import pytest

from conftest import params_7p5
from test_gpu_parity import Vd, _fresh_device, get, hip  # noqa: F401

pytestmark = pytest.mark.gpu

# Scaled agreement (max |difference| / max |sum|) of the fp32-stream product with the host's fp64 accumulation of the float-rounded tiles.  The fp64 form
# reaches, by dkmc_xtb_check_product at these shapes and width 16, PRODUCT_FP64_MEASURED (see test_product_on_the_fp32_image); the bound is 4 x that for
# the different summation order.
PRODUCT_FP64_MEASURED = {"2.5nm": 6.868e-16, "tile:2": 7.966e-16}       # (the image reached 4.5e-16 and 4.7e-16)


def _workload(name, cell_2p5, dev_7p5):
    from devicekmc_amd import params as pm, structure
    if name == "2.5nm":
        return cell_2p5, pm.KMCParameters()
    if name == "7.5nm":
        return dev_7p5, params_7p5()
    k = int(name.split(":")[1])
    return structure.tile_structure(cell_2p5, k, 25.575, 25.575, 1440), pm.KMCParameters().for_tiling(k)


def _test_panel(ns):
    r = np.arange(ns, dtype=np.uint64)[:, None]; v = np.arange(16, dtype=np.uint64)[None, :]
    h = (((r * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) ^ (v * np.uint64(40503))) >> np.uint64(20)
    return 0.25 + h.astype(np.float64) / 4096.0 + 0.125 * v.astype(np.float64)


def _host_products(tiles, tval, Q, ns_pad):
    """(product with the tiles rounded to float32, product with the fp64 tiles, |At| |v|), all accumulated in fp64, both triangles from one stored value"""
    out32 = np.zeros((ns_pad, 16)); out64 = np.zeros((ns_pad, 16)); outabs = np.zeros((ns_pad, 16))
    Qp = np.zeros((ns_pad, 16)); Qp[:Q.shape[0]] = Q
    B = tval.reshape(-1, 32, 32)
    for k, w, mask, soff in tiles:
        sl = 0
        for q in range(8):
            if not (int(mask) >> q) & 1:
                continue
            b = B[soff + sl]; sl += 1
            rows = slice(32 * k, 32 * k + 32); cols = slice(256 * w + 32 * q, 256 * w + 32 * q + 32)
            for o, bb in ((out32, b.astype(np.float32).astype(np.float64)), (out64, b), (outabs, np.abs(b))):
                o[rows] += bb @ (Qp[cols] if o is not outabs else np.abs(Qp[cols]))
                o[cols] += bb.T @ (Qp[rows] if o is not outabs else np.abs(Qp[rows]))
    return out32, out64, outabs


@pytest.mark.parametrize("which", ["2.5nm", "tile:2"])
def test_product_on_the_fp32_image(cell_2p5, dev_7p5, hip, which):
    """k_xtb_apply<..., float> on the 16 test vectors of dkmc_xtb_check_product, folded (dkmc_xtb_tile_product), against the host: the downloaded fp64
    tiles rounded with numpy.float32, accumulated in fp64 -- the same products, regrouped.  Both workloads hold partial tiles (mask != 0xff: census
    asserted), the padded last strip and empty runs.  Bound: 4 x what dkmc_xtb_check_product reaches for the fp64 form at the same shape (measured,
    PRODUCT_FP64_MEASURED, printed again by this test); every product of a 24-bit tile value and a 14-bit test value is exact in fp64, so only the order
    of the additions differs, as it does for the fp64 form.  Against the UNROUNDED fp64 product every element lies within 2^-23 (|At| |v|): derived --
    2^-24 per rounded entry, the rest for the rounding of the sums (32 k entries at most: far below 2^-24)."""
    from devicekmc_amd.lib import check
    host, L = hip
    structure, p = _workload(which, cell_2p5, dev_7p5)
    p.solve_heating_global = False
    try:
        L.dkmc_set_x_tile_f32(1)
        dev, sim, gb, _ = _fresh_device(structure, p, hip)
        dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, 0); dev.updatePower(gb, p, Vd)
        st = host.get_stats()
        assert st["x_tile_stream"] == 1 and st["x_tile_f32_bytes"] == 4096 * (st["xt_subblocks"] + 4), st
        h = (C.c_longlong * 11)()
        check(L.dkmc_xt_tile_census(h))
        assert h[8] > 0 and sum(h[1:8]) > 0, list(h)                     # full and partial tiles
        nt, nsub = C.c_longlong(0), C.c_longlong(0)
        check(L.dkmc_xt_get_tiles(C.byref(nt), C.byref(nsub), None, None))
        tiles = np.zeros((nt.value, 4), dtype=np.int32); tval = np.zeros(nsub.value * 1024)
        check(L.dkmc_xt_get_tiles(None, None, tiles.ctypes.data, tval.ctypes.data))
        ns = st["xt_ns"]; ns_pad = 256 * ((ns + 255) // 256)
        Q = _test_panel(ns)
        ref32, ref64, refabs = _host_products(tiles.astype(np.int64), tval, Q, ns_pad)
        d, a = C.c_double(-1), C.c_double(-1)
        check(L.dkmc_xtb_check_product(16, C.byref(d), C.byref(a)))
        print("%s: dkmc_xtb_check_product (fp64 form, width 16): %.3e scaled" % (which, d.value / a.value))
        for width in (16, 12, 8, 4):
            so = 4 * ((width + 3) // 4)
            got = {}
            for stored in (8, 4):
                out = np.zeros((ns, so))
                check(L.dkmc_xtb_tile_product(width, stored, out.ctypes.data))
                got[stored] = out
            big = np.abs(ref64[:ns, :so]).max()
            e64 = np.abs(got[8] - ref64[:ns, :so]).max() / big
            e32 = np.abs(got[4] - ref32[:ns, :so]).max() / big
            print("%s width %d: fp64 stream vs host %.3e, fp32 stream vs host (float-rounded tiles) %.3e scaled" % (which, width, e64, e32))
            assert e32 <= 4 * PRODUCT_FP64_MEASURED[which], (which, width, e32)
            assert np.all(np.abs(got[4] - ref64[:ns, :so]) <= 2.0 ** -23 * refabs[:ns, :so]), (which, width)
            assert not np.array_equal(got[4], got[8])                     # the image is really what was streamed
    finally:
        L.dkmc_set_x_tile_f32(1)


def _supersteps(structure, p, hip, mode, n=3):
    """n coupled supersteps with the switch at `mode`: event logs, sweeps, residuals, I_macro, site power, stats of every step"""
    host, L = hip
    L.dkmc_set_x_tile_f32(mode)
    dev, sim, gb, _ = _fresh_device(structure, p, hip)
    rec = []
    for k in range(n):
        dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, k)
        sim.executeKMCStep(gb, dev, want_log=True)
        dev.updatePower(gb, p, Vd)
        st = host.get_stats()
        rec.append(dict(log=np.array(sim.last_event_log).copy(), iters=st["cg_iters_X"], rr=st["cg_rr_X"], im=dev.imacro, power=get(gb, "site_power").copy(),
                        m=get(gb, "atom_virtual_potentials").copy(), pot=get(gb, "site_potential_charge").copy(), stream=st["x_tile_stream"],
                        f64_rounds=st["x_tile_f64_rounds"], bytes=st["x_tile_f32_bytes"], width=st["xb_width"], fallback=st["xb_fallback"]))
    return rec


# relative agreement of I_macro and site_power between the two settings: MEASURED on the three workloads below (largest: site_power of the first, cold
# superstep of 7.5nm, 1.970e-8; I_macro at most 5.3e-9; warm steps 1e-10 and below -- DESIGN section 4) x 10 for box-to-box summation differences.
# Two solves that both stop at a true residual of 1e-7 ... 8e-7 differ at this level whatever their arithmetic.
SOLVE_REL_MEASURED = 1.970e-8


@pytest.mark.parametrize("which", ["2.5nm", "7.5nm", "tile:3"])
def test_supersteps_with_and_without_the_fp32_image(cell_2p5, dev_7p5, hip, which):
    """Three coupled supersteps at the default tolerance with the switch at 0 and at 1: identical event sequences, sweeps per solve within +-1, no
    re-entry round with either setting, the true residual of column 0 (the fp64 pass that ends every solve) within the stop test both ways, I_macro and
    site_power within 10 x the measured relative difference."""
    structure, p = _workload(which, cell_2p5, dev_7p5)
    p.solve_heating_global = True
    host, L = hip
    try:
        a = _supersteps(structure, p, hip, 0)
        b = _supersteps(structure, p, hip, 1)
    finally:
        L.dkmc_set_x_tile_f32(1)
    worst = 0.0
    for k, (x, y) in enumerate(zip(a, b)):
        assert x["width"] == 16 and y["width"] == 16 and not x["fallback"] and not y["fallback"]
        assert x["stream"] == 0 and x["bytes"] == 0 and x["f64_rounds"] == 1, (k, x["stream"], x["bytes"], x["f64_rounds"])
        assert y["stream"] == 1 and y["bytes"] > 0 and y["f64_rounds"] == 0, (k, y["stream"], y["bytes"], y["f64_rounds"])
        assert np.array_equal(x["log"], y["log"]), k
        assert abs(x["iters"] - y["iters"]) <= 1, (k, x["iters"], y["iters"])
        assert x["rr"] <= p.cg_tol ** 2 and y["rr"] <= p.cg_tol ** 2, (k, x["rr"], y["rr"])
        di = abs(y["im"] / x["im"] - 1); dp = np.abs(y["power"] - x["power"]).max() / np.abs(x["power"]).max()
        worst = max(worst, di, dp)
        print("%s step %d: sweeps %d / %d, true residual %.3e / %.3e, rel dI_macro %.3e, rel dpower %.3e" % (which, k, x["iters"], y["iters"], np.sqrt(x["rr"]), np.sqrt(y["rr"]), di, dp))
    assert worst <= 10 * SOLVE_REL_MEASURED, (which, worst)


@pytest.mark.parametrize("which", ["7.5nm@1e-10", "2.5nm@log_revision"])
def test_gate_keeps_tight_tolerances_on_the_fp64_store(cell_2p5, dev_7p5, hip, which):
    """cg_tol below 1e-8: the switch changes nothing -- solution, sweeps and site arrays bit-identical, the stats report the fp64 stream, no image made."""
    host, L = hip
    if which.startswith("7.5nm"):
        structure, p = _workload("7.5nm", cell_2p5, dev_7p5); p.cg_tol = 1e-10
    else:
        structure, p = _workload("2.5nm", cell_2p5, dev_7p5); p = p.log_revision()
    p.solve_heating_global = True
    try:
        a = _supersteps(structure, p, hip, 0, n=2)
        b = _supersteps(structure, p, hip, 1, n=2)
    finally:
        L.dkmc_set_x_tile_f32(1)
    for x, y in zip(a, b):
        assert y["stream"] == 0 and y["bytes"] == 0
        assert x["iters"] == y["iters"] and x["rr"] == y["rr"] and x["im"] == y["im"]
        for f in ("log", "m", "power", "pot"):
            assert np.array_equal(x[f], y[f]), f


@pytest.mark.parametrize("how", ["x_poly(0)", "x_block(1)"])
def test_fallbacks_never_use_the_image(cell_2p5, dev_7p5, hip, how):
    """Preconditioner off, or the single-vector loop: bit-identical results between switch 0 and 1, no image allocated."""
    host, L = hip
    structure, p = _workload("7.5nm", cell_2p5, dev_7p5)
    p.solve_heating_global = True
    try:
        if how == "x_poly(0)":
            L.dkmc_set_x_poly(0)
        else:
            L.dkmc_set_x_block(1)
        a = _supersteps(structure, p, hip, 0, n=2)
        b = _supersteps(structure, p, hip, 1, n=2)
    finally:
        L.dkmc_set_x_tile_f32(1); L.dkmc_set_x_poly(8); L.dkmc_set_x_block(16)
    for x, y in zip(a, b):
        assert y["stream"] == 0 and y["bytes"] == 0
        assert x["iters"] == y["iters"] and x["rr"] == y["rr"] and x["im"] == y["im"]
        for f in ("log", "m", "power"):
            assert np.array_equal(x[f], y[f]), f


def test_slab_emulation_stays_on_the_fp64_store(dev_7p5, hip):
    """dkmc_xtb_emulate_slabs(2, ...) on the X a default solve left (image present): both of its loops -- the slab-distributed one and its one-GPU
    reference -- run on the fp64 store: same sweeps and the same difference, bit for bit, as on the X of a solve with the switch at 0."""
    from devicekmc_amd.lib import check
    host, L = hip
    p = params_7p5(); p.solve_heating_global = False
    got = []
    try:
        for mode in (0, 1):
            L.dkmc_set_x_tile_f32(mode)
            dev, sim, gb, _ = _fresh_device(dev_7p5, p, hip)
            dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, 0); dev.updatePower(gb, p, Vd)
            assert host.get_stats()["x_tile_stream"] == mode
            rd, it_s, it_r = C.c_double(-1), C.c_int(0), C.c_int(0)
            us, xd, mm = (C.c_double * 8)(), (C.c_longlong * 3)(), (C.c_int * 2)()
            check(L.dkmc_xtb_emulate_slabs(2, 16, 1e-6, -1, 0, C.byref(rd), C.byref(it_s), C.byref(it_r), us, xd, mm))
            assert host.get_stats()["x_tile_stream"] == 0
            got.append((rd.value, it_s.value, it_r.value))
    finally:
        L.dkmc_set_x_tile_f32(1)
    assert got[0] == got[1], got


def test_reentry_runs_on_the_fp64_store(dev_7p5, hip):
    """The first true-residual check is made to report "above tolerance" once, on the host side (dkmc_debug_fail_true_residual_once): the solve is
    re-entered, the second round runs on the fp64 store (x_tile_f64_rounds == 1 while the first round streamed the image) and the solve ends within the
    stop test."""
    host, L = hip
    p = params_7p5(); p.solve_heating_global = False
    try:
        L.dkmc_set_x_tile_f32(1)
        dev, sim, gb, _ = _fresh_device(dev_7p5, p, hip)
        dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, 0)
        L.dkmc_debug_fail_true_residual_once()
        dev.updatePower(gb, p, Vd)
        st = host.get_stats()
        assert st["x_tile_stream"] == 1 and st["x_tile_f64_rounds"] == 1, (st["x_tile_stream"], st["x_tile_f64_rounds"])
        assert st["xb_fallback"] == 0 and 0 <= st["cg_rr_X"] <= p.cg_tol ** 2, st["cg_rr_X"]
        dev.updatePower(gb, p, Vd)                                        # the aid is spent: an ordinary solve again
        st = host.get_stats()
        assert st["x_tile_stream"] == 1 and st["x_tile_f64_rounds"] == 0
    finally:
        L.dkmc_set_x_tile_f32(1)
