"""The norm stop test of the one-polynomial block-CG (dkmc_set_x_stop_form; csrc/xtb.hip: k_xtb_step1's partial sums, k_xtb_stop_norm).

Kernels, through dkmc_xtb_test_step1_norm on caller-given panels: the sum of Rt+(i, 0)^2 against the long-double sum over the Rt the aid returns, the
stop word it sets, and the panels against the same launch without the partial sums (bit for bit).

Solves, at 2.5nm (coupled supersteps: one cold, two warm) and on two synthetic lattice devices of tests/x_cases.py (a cold and a warm solve of one
state), one-polynomial form forced, degrees 4 and 10: form 0 leaves no trace of the feature, form 1 needs no more sweeps, no re-entry round, meets the
tolerance in the true residual and in the scaled residual on the exported X (10 cg_tol, I_macro within 1e-5 of the reference-order solve: what
tests/test_gpu_warm_start.py grants), and reports the norm of the Rt it stopped on.

Rounding of the sum (count c, |sum - exact| <= c u exact, every term positive): a thread squares and adds the 4 rows it stores per 16-row group over
G = ceil(groups / (4 workgroups)) groups, 4 G roundings of the additions + 1 of a product; the workgroup tree 8; k_xtb_stop_norm ceil(workgroups / 256)
additions per thread + its tree 8.  The reported norm is its square root (half the relative error, one more rounding): bound c u on the norm."""
import copy
import ctypes as C

import numpy as np
import pytest

import x_cases
from devicekmc_amd.lib import check, dkmc_xtb_ctrl
from test_gpu_block_cg_algebra import _p, _sranks, _step_mats
from test_gpu_parity import Vd, _fresh_device, _scaled_residual, get, hip, put  # noqa: F401
from test_gpu_x_poly_form_kernels import _ptrs, _step1

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
KAPPA = 1.0 / 1.5                     # the margin of these tests: the tightest of the three the default was chosen from


def _count(m):
    groups = -(-m // 16)
    wg = max(1, min(-(-groups // 4), 2048))
    return 4 * -(-groups // (4 * wg)) + 1 + 8 + -(-wg // 256) + 8


@pytest.fixture(autouse=True)
def _switches(hip):
    host, L = hip

    def reset():
        L.dkmc_set_x_stop_form(2); L.dkmc_set_x_stop_margin(0.0); L.dkmc_set_x_poly_form(2); L.dkmc_debug_set_x_poly1_degree(0)      # (margin 0: the default)
        L.dkmc_set_x_poly(8); L.dkmc_set_current_warm_start(1); L.dkmc_set_x_block(16)
    reset()
    yield
    reset()


# ---- kernels ------------------------------------------------------------------------------------------------------------------------------------------
def _step1_norm(L, it, mats, done, y0, panels, sc, nsrank, ns, qs, bound2, rr_in, prefill=(-1.0, -2.0, -3.0)):
    y0 = y0.copy(); panels = [p.copy() for p in panels]; qs = qs.copy()
    rec = np.array(prefill, dtype=np.float64); ctrl = dkmc_xtb_ctrl()
    check(L.dkmc_xtb_test_step1_norm(len(y0), it, _p(np.ascontiguousarray(mats)), done, _p(y0), _ptrs(panels), _p(sc), _p(nsrank), ns, _p(qs),
                                     bound2, rr_in, _p(rec), C.byref(ctrl)))
    return y0, panels, qs, rec, ctrl


# 131 155 rows: 8198 groups over 2048 workgroups of four waves -- a wave takes a second group, the last one ragged
@pytest.mark.parametrize("m", [1, 17, 4099, 131155])
def test_partial_sums_and_stop_word(hip, m):
    host, L = hip
    rng = np.random.default_rng(4100 + m)
    it = 6
    y0 = rng.standard_normal(m); sc = rng.uniform(0.5, 2.0, m)
    pan = [rng.standard_normal((m, 16)) for _ in range(6)]
    pan[4] *= 10.0 ** rng.uniform(-3, 3, (m, 1))                              # Rt: rows of very different size
    nsrank, ns = _sranks(m, "half", rng) if m > 1 else (np.zeros(1, dtype=np.int32), 1)
    qs0 = rng.standard_normal((ns, 16))
    mats = _step_mats(16, rng)
    plain = _step1(L, it, mats, 0, y0, pan, sc, nsrank, ns, qs0)
    y1, p1, qs1, rec, ctrl = _step1_norm(L, it, mats, 0, y0, pan, sc, nsrank, ns, qs0, 0.0, 0.375)
    # the panels are those of the launch without the partial sums, bit for bit
    for a, b in zip((y1, *p1, qs1), (plain[0], *plain[1], plain[2])):
        assert a.tobytes() == b.tobytes(), m
    exact = (p1[4][:, 0].astype(LD) ** 2).sum()
    c = _count(m)
    err = abs(LD(rec[0]) - exact) / (LD(U) * exact)
    print("x-stop sum m = %d: |gpu - ref| = %.2f u of %d" % (m, float(err), c))
    assert err <= c, (m, float(err), c)
    # negative control: the sum without the largest row is outside the bound
    big = np.max(p1[4][:, 0].astype(LD) ** 2)
    assert m == 1 or abs(LD(rec[0]) - (exact - big)) > c * LD(U) * exact
    # bound 0: no stop; the record holds the sum, rr as the kernel found it, 0
    assert rec[1] == 0.375 and rec[2] == 0.0 and ctrl.done == 0 and ctrl.iters == 0 and list(ctrl.rr) == [0.375, 0.375]
    # sum <= bound (equality included): the stop of sweep `it` -- done = it + 2, iters = it + 1, rr untouched
    for b2 in (rec[0], 2 * rec[0]):
        _, _, _, r2, c2 = _step1_norm(L, it, mats, 0, y0, pan, sc, nsrank, ns, qs0, b2, 0.375)
        assert r2[0] == rec[0] and r2[2] == 1.0 and c2.done == it + 2 and c2.iters == it + 1 and list(c2.rr) == [0.375, 0.375], (m, b2)
    _, _, _, r2, c2 = _step1_norm(L, it, mats, 0, y0, pan, sc, nsrank, ns, qs0, np.nextafter(rec[0], 0.0), 0.375)
    assert r2[2] == 0.0 and c2.done == 0
    # k_xtb_small of the sweep has stopped already (it + 2): the step runs, the norm is recorded, the stop stays the bound's
    y2, p2, _, r2, c2 = _step1_norm(L, it, mats, it + 2, y0, pan, sc, nsrank, ns, qs0, 2 * rec[0], 0.375)
    assert r2[0] == rec[0] and r2[2] == 0.0 and c2.done == it + 2 and c2.iters == 0 and p2[4].tobytes() == p1[4].tobytes()
    # an older stop word: neither kernel writes
    for done in (it + 1, 1):
        y2, p2, _, r2, c2 = _step1_norm(L, it, mats, done, y0, pan, sc, nsrank, ns, qs0, 2 * rec[0], 0.375)
        assert list(r2) == [-1.0, -2.0, -3.0] and c2.done == done and c2.iters == 0 and p2[4].tobytes() == pan[4].tobytes() and y2.tobytes() == y0.tobytes()


@pytest.mark.parametrize("m", [17, 4099])
def test_partial_sums_integer_rows_are_exact(hip, m):
    """Rt of integers in [-8, 8], c = 0: every square and every sum is an integer below 2^53, so the sum is exact whatever the order -- a row left out
    or counted twice cannot pass."""
    host, L = hip
    rng = np.random.default_rng(4200 + m)
    pan = [rng.standard_normal((m, 16)) for _ in range(6)]
    pan[4] = rng.integers(-8, 9, (m, 16)).astype(np.float64)
    mats = _step_mats(16, rng); mats[0] = 0.0
    nsrank = np.full(m, -1, dtype=np.int32)
    _, p1, _, rec, _ = _step1_norm(L, 0, mats, 0, np.zeros(m), pan, np.ones(m), nsrank, 0, np.zeros((0, 16)), 0.0, 1.0)
    assert p1[4].tobytes() == pan[4].tobytes()
    assert rec[0] == float((pan[4][:, 0].astype(np.int64) ** 2).sum()), m
    assert rec[0] != float((pan[4][1:, 0].astype(np.int64) ** 2).sum()) or pan[4][0, 0] == 0


def test_aid_and_switches_refuse_bad_arguments(hip):
    host, L = hip
    pan = [np.zeros((4, 16)) for _ in range(6)]
    y0 = np.zeros(4); sc = np.ones(4); nsr = np.full(4, -1, dtype=np.int32); mats = np.zeros((4, 16, 16)); rec = np.zeros(3); ctrl = dkmc_xtb_ctrl()
    for args in ((4, -1, _p(mats), 0, _p(y0), _ptrs(pan), _p(sc), _p(nsr), 0, None, 1.0, 1.0, _p(rec), C.byref(ctrl)),
                 (4, 0, _p(mats), 0, _p(y0), _ptrs(pan), _p(sc), _p(nsr), 0, None, 1.0, 1.0, None, C.byref(ctrl)),
                 (4, 0, _p(mats), 0, _p(y0), _ptrs(pan), _p(sc), _p(nsr), 0, None, 1.0, 1.0, _p(rec), None),
                 (0, 0, _p(mats), 0, _p(y0), _ptrs(pan), _p(sc), _p(nsr), 0, None, 1.0, 1.0, _p(rec), C.byref(ctrl))):
        assert L.dkmc_xtb_test_step1_norm(*args) != 0
        L.dkmc_clear_error()
    assert L.dkmc_get_x_stop_form() == 2 and L.dkmc_get_x_stop_margin() == 1.0      # the defaults (the fixture restored them)
    for form, want in ((7, 0), (1, 1), (2, 2), (-1, 0)):
        L.dkmc_set_x_stop_form(form)
        assert L.dkmc_get_x_stop_form() == want
    for bad in (0.0, -1.0, 1.5, float("nan")):
        L.dkmc_set_x_stop_margin(0.8); L.dkmc_set_x_stop_margin(bad)
        assert L.dkmc_get_x_stop_margin() == 1.0
    L.dkmc_set_x_stop_margin(0.8)
    assert L.dkmc_get_x_stop_margin() == 0.8


# ---- solves -----------------------------------------------------------------------------------------------------------------------------------------------
def _stop_info(L):
    f = C.c_int(-1); a = [C.c_double(), C.c_double(), C.c_double()]
    rc = L.dkmc_get_x_stop_info(C.byref(f), C.byref(a[0]), C.byref(a[1]), C.byref(a[2]))
    return dict(rc=rc, fired=f.value, norm=a[0].value, rz=a[1].value, true=a[2].value)


def _record(host, L, dev, gb, p, vd):
    """the solve just made, then two more of the same state that check it: the scaled residual on the exported X, and I_macro of the reference-order solve
    (single-vector loop, reference start vector; the private warm-start copy is left alone in that mode)"""
    st = host.get_stats()
    r = dict(m=get(gb, "atom_virtual_potentials").copy(), power=get(gb, "site_power").copy(), im=dev.imacro, iters=st["cg_iters_X"], rr=st["cg_rr_X"],
             f64=st["x_tile_f64_rounds"], stream=st["x_tile_stream"], one=L.dkmc_get_x_poly_form_used(), products=L.dkmc_get_x_poly_products(),
             fallback=st["xb_fallback"], info=_stop_info(L))
    rows = dev.N_atom + 1
    rt0 = np.zeros(rows)
    check(L.dkmc_debug_get_x_stop_rt0(rows, _p(rt0)))
    r["rt0"] = rt0
    # the solution itself: the private warm-start copy (unscaled; the buffer is G0-scaled and, with global heating on, overwritten behind the solve)
    w = np.zeros(rows); nw = C.c_int(-1)
    check(L.dkmc_get_current_warm_vector(C.byref(gb.c), w.ctypes.data_as(C.c_void_p), rows, C.byref(nw)))
    assert nw.value == rows
    rp, ci, data = host.get_last_X()
    r["res_X"] = _scaled_residual(rp, ci, data, np.concatenate([w, np.zeros(max(len(rp) - 1 - rows, 0))]), 1.0, p.X_loop_G, vd)      # (a ground row, if exported: 0)
    try:
        L.dkmc_set_current_warm_start(0); L.dkmc_set_x_block(1)
        dev.updatePower(gb, p, vd)
        r["im_ref"] = dev.imacro
    finally:
        L.dkmc_set_current_warm_start(1); L.dkmc_set_x_block(16)
    put(gb, "atom_virtual_potentials", r["m"])
    return r


def _solves(which, cell_2p5, hip, fail_at=None):
    """2.5nm: three coupled supersteps; a synthetic case: a cold and a warm solve of its state, at the library's default tolerance 1e-6 (the cases' own 1e-10 leaves no fp32 image to stream)"""
    host, L = hip
    rec = []
    if which == "2.5nm":
        from devicekmc_amd import params as pm
        p = pm.KMCParameters(); p.solve_heating_global = True
        dev, sim, gb, _ = _fresh_device(cell_2p5, p, hip)
        for k in range(3):
            dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, k)
            sim.executeKMCStep(gb, dev, want_log=True)
            if fail_at == k:
                L.dkmc_debug_fail_true_residual_once()
            dev.updatePower(gb, p, Vd)
            rec.append(_record(host, L, dev, gb, p, Vd)); rec[-1]["log"] = np.array(sim.last_event_log).copy()
        return rec, p.cg_tol
    s, p, vd, cb, counts = x_cases.make_case(which)
    p = copy.deepcopy(p); p.cg_tol = 1e-6; p.solve_heating_global = True
    dev = host.Device(s, p)
    dev.site_CB_edge = cb.copy()
    gb = dev.make_gpubuf("cuda:0")
    put(gb, "site_CB_edge", cb)
    dev.updateCharge(gb)
    for k in range(2):
        if fail_at == k:
            L.dkmc_debug_fail_true_residual_once()
        dev.updatePower(gb, p, vd)
        rec.append(_record(host, L, dev, gb, p, vd)); rec[-1]["log"] = np.zeros(0)
    return rec, p.cg_tol


def _same_bits(a, b):
    return (a["iters"] == b["iters"] and a["rr"] == b["rr"] and a["im"] == b["im"] and np.array_equal(a["m"], b["m"]) and np.array_equal(a["power"], b["power"])
            and np.array_equal(a["log"], b["log"]))


@pytest.mark.parametrize("n", [4, 10])
@pytest.mark.parametrize("which", ["2.5nm", "n305_v3", "n64_v257"])
def test_solves_form_0_and_form_1(cell_2p5, hip, which, n):
    host, L = hip
    L.dkmc_set_x_poly_form(1); L.dkmc_debug_set_x_poly1_degree(n)
    L.dkmc_set_x_stop_form(0)
    ref, tol = _solves(which, cell_2p5, hip)
    L.dkmc_set_x_stop_form(1); L.dkmc_set_x_stop_margin(KAPPA)
    got, _ = _solves(which, cell_2p5, hip)
    L.dkmc_set_x_stop_margin(1e-9)                                            # the norm test cannot fire before the bound does
    tiny, _ = _solves(which, cell_2p5, hip)
    L.dkmc_set_x_stop_form(0 if n == 4 else 2); L.dkmc_set_x_stop_margin(KAPPA)      # (2: these systems lie below the size gate of the default)
    back, _ = _solves(which, cell_2p5, hip)
    rows = len(ref[0]["rt0"]); c = _count(rows)
    same_start = True                                                         # form 1 has started every solve so far from form 0's bits
    for k, (x, y, t, z) in enumerate(zip(ref, got, tiny, back)):
        di = abs(y["im"] / x["im"] - 1); dp = np.abs(y["power"] - x["power"]).max() / np.abs(x["power"]).max()
        print("x-stop %s n = %d solve %d: sweeps %d (form 0: %d), fired %d (form 0: %d), norm at the stop %.3e, (Rt'Z)_00 %.3e (form 0: %.3e), true residual %.3e "
              "(form 0: %.3e) of %.0e, on X %.3e, rel dI_macro %.3e, rel dpower %.3e"
              % (which, n, k, y["iters"], x["iters"], y["info"]["fired"], x["info"]["fired"], y["info"]["norm"], y["info"]["rz"], x["info"]["rz"], y["info"]["true"],
                 x["info"]["true"], tol, y["res_X"], di, dp))
    for k, (x, y, t, z) in enumerate(zip(ref, got, tiny, back)):
        for r in (x, y, t, z):
            assert r["one"] == 1 and r["products"] == n and r["fallback"] == 0 and r["info"]["rc"] == 0, (k, r["one"], r["products"])
        # form 0: today's test alone -- the same bits before and after form 1 ran in the process, the bound's stop, no norm measured
        assert _same_bits(x, z), (which, n, k)
        assert x["info"]["fired"] == 1 and x["info"]["norm"] == -1.0 and z["info"]["fired"] == 1
        assert x["info"]["true"] == np.sqrt(x["rr"])
        # a margin the norm cannot reach first: form 0's sweeps, stop and bits, with the norm reported beside it
        assert _same_bits(x, t) and t["info"]["fired"] == 1 and t["info"]["norm"] > 1e-9 * tol, (which, n, k, t["info"])
        # form 1
        assert y["iters"] <= x["iters"], (which, n, k)
        assert y["f64"] == (0 if y["stream"] == 1 else 1), (which, n, k, y["f64"], y["stream"])      # no re-entry round
        assert 0 <= y["rr"] <= tol ** 2 and y["info"]["true"] == np.sqrt(y["rr"]), (which, n, k, y["rr"])
        assert y["info"]["fired"] in (1, 2)
        if y["info"]["fired"] == 2:
            assert y["info"]["norm"] <= KAPPA * tol and (not same_start or y["iters"] < x["iters"]), (which, n, k, y["info"], y["iters"], x["iters"])
            same_start = False
        elif same_start:
            assert _same_bits(x, y), (which, n, k)                            # the bound fired first: form 0's solve
        for r in (y, t):
            exact = np.sqrt((r["rt0"].astype(LD) ** 2).sum())
            err = abs(LD(r["info"]["norm"]) - exact) / (LD(U) * exact)
            print("x-stop %s n = %d solve %d: reported norm against the exported Rt: %.2f u of %d" % (which, n, k, float(err), c))
            assert err <= c, (which, n, k, float(err), c)
        assert np.array_equal(x["log"], y["log"])
        assert y["res_X"] <= 10 * tol and x["res_X"] <= 10 * tol, (which, n, k, y["res_X"])
        assert abs(y["im"] / y["im_ref"] - 1) <= 1e-5 and abs(x["im"] / x["im_ref"] - 1) <= 1e-5, (which, n, k)
        assert np.all(np.isfinite(y["m"]))


@pytest.mark.parametrize("which", ["2.5nm", "n64_v257"])
def test_a_failed_true_residual_check_still_re_enters(cell_2p5, hip, which):
    """dkmc_debug_fail_true_residual_once in front of the warm solve under form 1: the solve is re-entered (a round on the fp64 store, stopping on the bound
    alone) and converges."""
    host, L = hip
    L.dkmc_set_x_poly_form(1); L.dkmc_debug_set_x_poly1_degree(10); L.dkmc_set_x_stop_form(1)
    got, tol = _solves(which, cell_2p5, hip, fail_at=1)
    y = got[1]
    print("x-stop %s re-entry: sweeps %d, fp64 rounds %d, fired %d, true residual %.3e, on X %.3e" % (which, y["iters"], y["f64"], y["info"]["fired"], y["info"]["true"], y["res_X"]))
    assert y["f64"] >= 1 and y["stream"] == 1, (y["f64"], y["stream"])
    assert y["info"]["fired"] == 1 and y["info"]["norm"] == -1.0             # the last round stopped on the bound alone
    assert 0 <= y["rr"] <= tol ** 2 and y["res_X"] <= 10 * tol
    assert abs(y["im"] / y["im_ref"] - 1) <= 1e-5
    assert got[0]["f64"] == 0
