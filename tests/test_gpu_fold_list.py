"""The list fold of the tile launch's row partial sums in the one-GPU preconditioned block-CG (dkmc_set_x_fold_form; csrc/xtb.hip: xtb_wlist_sum2,
k_xtb_fold_rows; the lists: k_xt_wrange in csrc/xt.hip, xt_live_build in csrc/xt_live.h).  Form 1 (default) adds only the cells of the launch view's
tiles and zeroes nothing; form 0 is the range fold over a per-solve memset and k_xtl_zero_dead, kept as the same-process reference.  The contract is
BITS: every case compares form 1 with form 0 byte for byte, from one saved state with the start vector put back before each solve.

Shapes: 2.5nm (9 399 sites, 928 members of S: 29 full row blocks by 4 windows, full and partial tiles) and tile:3 (84 591 sites, 8 360 members: 262 row
blocks by 33 windows, the last one partial, row blocks with more than 16 listed windows -- the 16-wide batches and their predicated tail -- and ranges
with absent cells; all asserted from the library's lists).  The live view is forced by an explicit threshold, the median of the tiles' largest scaled
magnitudes (as tests/test_gpu_tile_drop.py), which puts dead tiles inside live ranges (asserted at tile:3; 2.5nm has 4 windows and none); at tile:3 it
is raised until one row block has an empty live list beside a non-empty full one (measured: median 4.0e-7, used 1.6e-6, 675 of 2 352 tiles live).
Every solve starts from the saved solution perturbed by 1e-3 relative, so the loop runs 7 to 23 sweeps per case.

One vector group for the one-column products: in form 1 the first product A y0 and the true-residual pass run k_xtb_apply and the fold at width 4, in
form 0 at width 16, so every byte comparison below also holds the width-4 launches to the width-16 ones; test_width4_product_against_the_host checks the
width-4 instantiation against the host on its own."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import Vd, _fresh_device, get, hip  # noqa: F401
from test_gpu_tile_drop import _info
from test_gpu_tile_f32 import PRODUCT_FP64_MEASURED, _workload

pytestmark = pytest.mark.gpu

SITE_FIELDS = ("site_element", "site_charge", "site_potential_boundary", "site_potential_charge", "site_power", "site_temperature", "site_CB_edge")


def _defaults(L):
    L.dkmc_set_x_fold_form(1); L.dkmc_debug_poison_fold_cells(0); L.dkmc_set_x_tile_drop(0.0); L.dkmc_set_x_tile_drop_unit(0); L.dkmc_set_x_poly_form(2)
    L.dkmc_set_current_warm_start(1)


def test_default_and_clamping(hip):
    host, L = hip
    try:
        assert L.dkmc_get_x_fold_form() == 1                               # a fresh library, and what every test leaves behind
        L.dkmc_set_x_fold_form(0)
        assert L.dkmc_get_x_fold_form() == 0
        for v in (1, 2, -1, 7):
            L.dkmc_set_x_fold_form(0); L.dkmc_set_x_fold_form(v)
            assert L.dkmc_get_x_fold_form() == 1, v
    finally:
        _defaults(L)


def _lists(L, live):
    """the window lists of the full (live 0) or the last solve's live view (1): a list of ascending int arrays, one per row block"""
    from devicekmc_amd.lib import check
    nK, nW = C.c_int(0), C.c_int(0)
    check(L.dkmc_xt_get_fold_lists(live, C.byref(nK), C.byref(nW), None))
    rows = np.zeros((nK.value, nW.value + 1), dtype=np.int32)
    check(L.dkmc_xt_get_fold_lists(live, C.byref(nK), C.byref(nW), rows.ctypes.data))
    assert rows[:, 0].min() >= 0 and rows[:, 0].max() <= nW.value
    return [rows[k, 1:1 + rows[k, 0]].copy() for k in range(nK.value)], nW.value


def _expected(tiles, keep, nK):
    out = [[] for _ in range(nK)]
    for (k, w, _, _), f in zip(tiles, keep):
        if f:
            out[k].append(w)
    return [np.sort(np.array(x, dtype=np.int32)) for x in out]


def _live_flags(L, theta, nt):
    from devicekmc_amd.lib import check
    flags = np.zeros(nt, dtype=np.int32)
    check(L.dkmc_xt_get_live(theta, flags.ctypes.data, None))
    return flags != 0


def _state(which, cell_2p5, dev_7p5, hip):
    """The device after one current solve at the defaults: the tile list, the tiles' largest scaled magnitudes (host, as test_gpu_tile_drop.py computes
    them), the threshold of the live-view cases and the start vector of the NEXT solve.  Computed once per shape, shared, left unchanged."""
    from devicekmc_amd.lib import check
    host, L = hip
    structure, p = _workload(which, cell_2p5, dev_7p5)
    p.solve_heating_global = False
    _defaults(L)
    dev, sim, gb, _ = _fresh_device(structure, p, hip, warm=1)
    dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, 0); dev.updatePower(gb, p, Vd)
    st = host.get_stats()
    nt, nsub = C.c_longlong(0), C.c_longlong(0)
    check(L.dkmc_xt_get_tiles(C.byref(nt), C.byref(nsub), None, None))
    tiles = np.zeros((nt.value, 4), dtype=np.int32); tval = np.zeros(nsub.value * 1024)
    check(L.dkmc_xt_get_tiles(None, None, tiles.ctypes.data, tval.ctypes.data))
    ns = st["xt_ns"]
    sS = np.zeros(ns)
    check(L.dkmc_xt_get_live(1.0, None, sS.ctypes.data))
    sSp = np.zeros(256 * ((ns + 255) // 256) + 256); sSp[:ns] = sS
    B = np.abs(tval.reshape(-1, 32, 32)); del tval
    tmax = np.zeros(nt.value)
    for t, (k, w, mask, soff) in enumerate(tiles.astype(np.int64)):
        sl = 0
        for q in range(8):
            if (int(mask) >> q) & 1:
                tmax[t] = max(tmax[t], ((sSp[32 * k:32 * k + 32, None] * B[soff + sl]) * sSp[None, 256 * w + 32 * q:256 * w + 32 * q + 32]).max())
                sl += 1
    del B
    full, nW = _lists(L, 0)
    nK = len(full)
    theta = float(np.median(tmax))
    if which == "tile:3":
        # a row block whose live list is empty while its full one is not: from the library's own masks; raise the threshold until one exists
        while True:
            live = _expected(tiles, _live_flags(L, theta, nt.value), nK)
            if any(len(a) > 0 and len(b) == 0 for a, b in zip(full, live)):
                break
            assert theta < 1e-4, "no row block loses all its tiles below the largest threshold the switch keeps"
            theta = min(theta * 4.0, 1e-4)
        print("tile:3: threshold used %.3e (median of the tiles' largest scaled magnitudes %.3e)" % (theta, float(np.median(tmax))))
    n = C.c_int(0)
    check(L.dkmc_get_current_warm_vector(C.byref(gb.c), None, 0, C.byref(n)))
    W = np.zeros(n.value)
    check(L.dkmc_get_current_warm_vector(C.byref(gb.c), W.ctypes.data, n.value, C.byref(n)))
    assert n.value > 0
    # (the solution itself would end every case after one sweep: a deterministic relative perturbation of 1e-3 gives the loop sweeps to run)
    W = W * (1.0 + 1e-3 * np.cos(np.arange(n.value, dtype=np.float64)))
    return dict(which=which, dev=dev, gb=gb, p=p, tiles=tiles, ns=ns, nK=nK, nW=nW, full=full, theta=theta, W=W, cases={})


@pytest.fixture(scope="module")
def state_2p5(cell_2p5, dev_7p5, hip):
    return _state("2.5nm", cell_2p5, dev_7p5, hip)


@pytest.fixture(scope="module")
def state_t3(cell_2p5, dev_7p5, hip):
    return _state("tile:3", cell_2p5, dev_7p5, hip)


@pytest.fixture(params=["2.5nm", "tile:3"])
def state(request):
    return request.getfixturevalue("state_2p5" if request.param == "2.5nm" else "state_t3")


def _solve(s, hip, fold, theta, poly, poison=0, unit=0, fail_once=False, keep=True):
    """the current solve of the saved state from the saved start vector with the switches as given; form-0 results are kept per case (the reference is
    computed once and shared)"""
    from devicekmc_amd.lib import check
    host, L = hip
    key = (fold, theta, poly, poison, unit, fail_once)
    if keep and key in s["cases"]:
        return s["cases"][key]
    check(L.dkmc_set_current_warm_vector(C.byref(s["gb"].c), s["W"].ctypes.data, len(s["W"])))
    L.dkmc_set_x_fold_form(fold); L.dkmc_debug_poison_fold_cells(poison); L.dkmc_set_x_tile_drop(theta); L.dkmc_set_x_tile_drop_unit(unit)
    L.dkmc_set_x_poly_form(poly)
    if fail_once:
        L.dkmc_debug_fail_true_residual_once()
    s["dev"].updatePower(s["gb"], s["p"], Vd)
    st = host.get_stats()
    r = dict(m=get(s["gb"], "atom_virtual_potentials").copy(), power=get(s["gb"], "site_power").copy(), im=np.float64(s["dev"].imacro),
             iters=st["cg_iters_X"], rr=np.float64(st["cg_rr_X"]), f64=st["x_tile_f64_rounds"], info=_info(L), one=L.dkmc_get_x_poly_form_used(),
             stream=st["x_tile_stream"])
    if keep:
        s["cases"][key] = r
    return r


def _assert_same_bits(a, b, what):
    for f in ("m", "power"):
        assert np.all(np.isfinite(b[f])), (what, f)
        assert a[f].tobytes() == b[f].tobytes(), (what, f)
    for f in ("im", "rr"):
        assert np.isfinite(b[f]) and a[f].tobytes() == b[f].tobytes(), (what, f, a[f], b[f])
    assert a["iters"] == b["iters"] and a["f64"] == b["f64"], (what, a["iters"], b["iters"], a["f64"], b["f64"])


@pytest.mark.parametrize("unit", [0, 1])
def test_lists_are_the_windows_of_the_tiles(state, hip, unit):
    """Every list equals the ascending windows of its row block's tiles: the full view's against the tile list, the live view's against the live flags of
    the same threshold -- with whole tiles (unit 0) and with sub-blocks (unit 1) dropped: the set of live tiles is the same in both."""
    host, L = hip
    s = state
    try:
        r = _solve(s, hip, 1, s["theta"], 2, unit=unit, keep=False)
        assert r["info"][0] == 1 and r["info"][2] < r["info"][1], r["info"]
        full, nW = _lists(L, 0)
        live, _ = _lists(L, 1)
        flags = _live_flags(L, s["theta"], len(s["tiles"]))
    finally:
        _defaults(L)
    exp_full = _expected(s["tiles"], np.ones(len(s["tiles"]), dtype=bool), s["nK"])
    exp_live = _expected(s["tiles"], flags, s["nK"])
    assert flags.sum() == r["info"][2]
    for k in range(s["nK"]):
        assert np.array_equal(full[k], exp_full[k]), (k, full[k], exp_full[k])
        assert np.array_equal(live[k], exp_live[k]), (k, live[k], exp_live[k])
    assert 32 * s["nK"] >= s["ns"] > 32 * (s["nK"] - 1)
    print("%s: %d members of S, %d in the last row block" % (s["which"], s["ns"], s["ns"] - 32 * (s["nK"] - 1)))
    if s["which"] == "tile:3":
        assert s["ns"] % 32 != 0                                            # a partial last row block
        assert max(len(a) for a in full) > 16                               # a second batch of 16 and its predicated tail
        assert any(0 < len(a) < a[-1] + 1 - a[0] for a in full)             # absent cells inside a range
        assert any(len(a) > 0 and len(b) == 0 for a, b in zip(full, live))  # a row block that lost every tile
    holes = sum(1 for a, b in zip(full, live) if len(b) > 0 and any(b[0] < w < b[-1] and w not in b for w in a))
    print("%s unit %d: %d row blocks, %d windows, %d of %d tiles live, row blocks with a dead tile inside their live range: %d" %
          (s["which"], unit, s["nK"], nW, flags.sum(), len(flags), holes))
    if s["which"] == "tile:3":
        assert holes > 0                                                    # dead tiles inside live ranges (2.5nm has 4 windows: printed only)


@pytest.mark.parametrize("poly", [0, 1], ids=["split", "one-polynomial"])
@pytest.mark.parametrize("view", ["full", "live"])
def test_same_bits_as_the_range_fold(state, hip, view, poly):
    """The same current solve from the same start vector with form 0 and with form 1 (and, in form 1, with every cell of the partial-sum array set to NaN
    first: nothing outside a list is read): solution, site_power, I_macro, sweeps, true residual and fp64 rounds byte for byte.  Form 1 runs the first
    product and the true-residual pass at width 4, form 0 at width 16."""
    host, L = hip
    s = state
    theta = s["theta"] if view == "live" else 0.0
    try:
        a = _solve(s, hip, 0, theta, poly)
        b = _solve(s, hip, 1, theta, poly, keep=False)
        c = _solve(s, hip, 1, theta, poly, poison=1, keep=False)
    finally:
        _defaults(L)
    print("%s %s view, poly form %d: sweeps %d, true residual %.3e, fp64 rounds %d, live info %s" % (s["which"], view, poly, a["iters"], np.sqrt(a["rr"]), a["f64"], b["info"]))
    assert a["iters"] > 1                                                   # the sweeps' fold ran more than once
    for r in (a, b, c):
        assert r["one"] == poly and r["stream"] == 1 and r["info"][0] == (1 if view == "live" else 0), (r["one"], r["stream"], r["info"])
        assert 0 <= r["rr"] <= s["p"].cg_tol ** 2
    _assert_same_bits(a, b, "form 1")
    _assert_same_bits(a, c, "form 1 over NaN cells")


def test_reentry_on_the_full_list(state, hip):
    """dkmc_debug_fail_true_residual_once with the live view: the re-entry round runs on the fp64 store and the full view's list, converges, and gives form
    0's re-entry result byte for byte (over NaN cells too)."""
    host, L = hip
    s = state
    try:
        a = _solve(s, hip, 0, s["theta"], 2, fail_once=True)
        b = _solve(s, hip, 1, s["theta"], 2, fail_once=True, keep=False)
        c = _solve(s, hip, 1, s["theta"], 2, poison=1, fail_once=True, keep=False)
    finally:
        _defaults(L)
    for r in (a, b, c):
        assert r["info"][0] == 1 and r["f64"] == 1 and 0 <= r["rr"] <= s["p"].cg_tol ** 2, (r["info"], r["f64"], r["rr"])
    _assert_same_bits(a, b, "re-entry")
    _assert_same_bits(a, c, "re-entry over NaN cells")


def test_coupled_supersteps_tile3(cell_2p5, dev_7p5, hip):
    """Three coupled supersteps at tile:3, warm start on, the live view at 1e-10, with form 0 and with form 1: dt, the events, I_macro and every site field
    a caller of the superstep receives are byte-identical."""
    host, L = hip
    structure, p = _workload("tile:3", cell_2p5, dev_7p5)
    p.solve_heating_global = True
    runs = []
    try:
        for fold in (0, 1):
            _defaults(L)
            L.dkmc_set_x_fold_form(fold); L.dkmc_set_x_tile_drop(1e-10)
            dev, sim, gb, _ = _fresh_device(structure, p, hip, warm=1)
            rec = []
            for k in range(3):
                dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, k)
                _, dt = sim.executeKMCStep(gb, dev, want_log=True)
                dev.updatePower(gb, p, Vd)
                dev.updateTemperature(gb, p, dt)
                st = host.get_stats()
                rec.append(dict(dt=np.float64(dt), im=np.float64(dev.imacro), T=np.float64(dev.T_bg), log=np.array(sim.last_event_log).copy(), iters=st["cg_iters_X"],
                                info=_info(L), fields={f: get(gb, f).copy() for f in SITE_FIELDS}))
            runs.append(rec)
            del dev, sim, gb
    finally:
        _defaults(L)
    for k, (x, y) in enumerate(zip(*runs)):
        print("tile:3 step %d: sweeps %d / %d, live info %s" % (k, x["iters"], y["iters"], y["info"]))
        assert y["info"][0] == 1 and x["info"] == y["info"], (k, x["info"], y["info"])
        assert x["iters"] == y["iters"], k
        for f in ("dt", "im", "T"):
            assert np.isfinite(y[f]) and x[f].tobytes() == y[f].tobytes(), (k, f, x[f], y[f])
        assert np.array_equal(x["log"], y["log"]), k
        for f in SITE_FIELDS:
            assert x["fields"][f].tobytes() == y["fields"][f].tobytes(), (k, f)


def test_width4_product_against_the_host(state, hip):
    """dkmc_xtb_check_product(4, ...): the one-group instantiation of the tile x panel kernel (what form 1 launches for the one-column products) against 4
    passes of the single-vector tile kernel, scaled by the largest sum.  Bound: the one test_gpu_tile_f32.py uses, 4 x PRODUCT_FP64_MEASURED (what the
    fp64 form reaches at width 16; columns 0-3 are formed by the same instructions at either width, the factor covers the smaller largest sum of four
    columns).  tile:3 has no measured entry there: a row's sum has 9 / 4 the terms of tile:2's (members of S in proportion to the lateral area) and a
    rounding bound grows at most linearly with the terms, so tile:2's figure x 9 / 4 stands in."""
    from devicekmc_amd.lib import check
    host, L = hip
    s = state
    bound = 4 * (PRODUCT_FP64_MEASURED["2.5nm"] if s["which"] == "2.5nm" else PRODUCT_FP64_MEASURED["tile:2"] * 9 / 4)
    try:
        _solve(s, hip, 1, 0.0, 2, keep=False)                               # the resident X of this shape
        d, a = C.c_double(-1), C.c_double(-1)
        check(L.dkmc_xtb_check_product(4, C.byref(d), C.byref(a)))
    finally:
        _defaults(L)
    print("%s: dkmc_xtb_check_product(4): %.3e scaled (largest sum %.3e), bound %.3e" % (s["which"], d.value / a.value, a.value, bound))
    assert a.value > 0 and 0 <= d.value / a.value <= bound
