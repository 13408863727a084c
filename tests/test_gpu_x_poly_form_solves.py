"""The one-polynomial form of the preconditioned block-CG (dkmc_set_x_poly_form; csrc/xtb.hip) in coupled supersteps against the split form at the same
level d: same events, every true residual within the stop test, I_macro and site power within the project's bound between two preconditioners, no
fallback, no more sweeps than the split form plus a margin, and n(d) N products per sweep against 2 d.  Then a converged tolerance from a zero start, and
the switch: a pinned degree keeps the split form's bits under form 2."""
import numpy as np
import pytest

from test_gpu_parity import Vd, _fresh_device, get, hip  # noqa: F401
from test_gpu_tile_f32 import _workload
from test_gpu_x_poly_auto import REL_BETWEEN_DEGREES

pytestmark = pytest.mark.gpu

N_OF_D = {8: 10, 16: 18}            # the measured degree map (csrc/xtb_precond.h: xtb_poly1_degree)


def _supersteps(structure, p, hip, n=3, warm=None):
    host, L = hip
    dev, sim, gb, _ = _fresh_device(structure, p, hip, warm=warm)
    rec = []
    for k in range(n):
        dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, k)
        sim.executeKMCStep(gb, dev, want_log=True)
        dev.updatePower(gb, p, Vd)
        st = host.get_stats()
        rec.append(dict(log=np.array(sim.last_event_log).copy(), im=dev.imacro, power=get(gb, "site_power").copy(), iters=st["cg_iters_X"], rr=st["cg_rr_X"],
                        used=st["xb_poly_used"], width=st["xb_width"], fallback=st["xb_fallback"], stream=st["x_tile_stream"], f64=st["x_tile_f64_rounds"],
                        one=L.dkmc_get_x_poly_form_used(), products=L.dkmc_get_x_poly_products()))
    return rec


def _restore(L):
    L.dkmc_set_x_poly_form(2); L.dkmc_debug_set_x_poly1_degree(0); L.dkmc_set_x_poly(8); L.dkmc_set_current_warm_start(1)


@pytest.mark.parametrize("d", [8, 16])
@pytest.mark.parametrize("which", ["2.5nm", "tile:2", "7.5nm"])
def test_supersteps_against_the_split_form(cell_2p5, dev_7p5, hip, which, d):
    """Three coupled supersteps (one cold, two warm) at the default tolerance, form 0 at level d against form 1 at n(d).
    Measured on an MI355X, sweeps per step split / one polynomial: 2.5nm d = 8: 9 6 5 / 10 6 5, d = 16: 9 5 5 / 10 6 5; tile:2 d = 8: 12 8 8 / 12 8 8,
    d = 16: 10 7 7 / 11 7 7; 7.5nm d = 8: 13 10 10 / 13 10 10, d = 16: 11 8 8 / 11 8 8 (bound: split + max(2, 10 %)); I_macro within 2.9e-9, site power
    within 4.6e-9 (bound 1e-5); DESIGN 4."""
    host, L = hip
    structure, p = _workload(which, cell_2p5, dev_7p5)
    p.solve_heating_global = True
    try:
        L.dkmc_set_x_poly(d); L.dkmc_set_x_poly_form(0)
        ref = _supersteps(structure, p, hip)
        L.dkmc_set_x_poly_form(1)
        got = _supersteps(structure, p, hip)
    finally:
        _restore(L)
    for k, (x, y) in enumerate(zip(ref, got)):
        di = abs(y["im"] / x["im"] - 1); dp = np.abs(y["power"] - x["power"]).max() / np.abs(x["power"]).max()
        print("%s d = %d step %d: sweeps %d (split: %d), N products per sweep %d (split: %d), true residual %.3e (split: %.3e), rel dI_macro %.3e, rel dpower %.3e"
              % (which, d, k, y["iters"], x["iters"], y["products"], x["products"], np.sqrt(max(y["rr"], 0.0)), np.sqrt(max(x["rr"], 0.0)), di, dp))
    for k, (x, y) in enumerate(zip(ref, got)):
        assert x["used"] == d and x["one"] == 0 and x["products"] == 2 * d, (k, x["used"], x["one"], x["products"])
        assert y["used"] == d and y["one"] == 1 and y["products"] == N_OF_D[d], (k, y["used"], y["one"], y["products"])
        assert x["width"] == 16 and y["width"] == 16 and x["fallback"] == 0 and y["fallback"] == 0
        assert np.array_equal(x["log"], y["log"]), (which, d, k)
        assert 0 <= x["rr"] <= p.cg_tol ** 2 and 0 <= y["rr"] <= p.cg_tol ** 2, (k, x["rr"], y["rr"])
        di = abs(y["im"] / x["im"] - 1); dp = np.abs(y["power"] - x["power"]).max() / np.abs(x["power"]).max()
        assert di <= REL_BETWEEN_DEGREES and dp <= REL_BETWEEN_DEGREES, (which, d, k, di, dp)
        assert y["iters"] <= x["iters"] + max(2, 0.1 * x["iters"]), (which, d, k, y["iters"], x["iters"])


def test_zero_start_at_a_converged_tolerance(cell_2p5, hip):
    """2.5nm, cg_tol 1e-10, zero start: no fp32 image exists, the sweeps run on the fp64 store; the solve ends solved and its true scaled residual is no
    worse than twice what the split form reaches on the same state."""
    from devicekmc_amd import params as pm
    host, L = hip
    p = pm.KMCParameters(); p.solve_heating_global = True; p.cg_tol = 1e-10
    try:
        L.dkmc_set_x_poly(8); L.dkmc_set_x_poly_form(0)
        x = _supersteps(cell_2p5, p, hip, n=1, warm=0)[0]
        L.dkmc_set_x_poly_form(1)
        y = _supersteps(cell_2p5, p, hip, n=1, warm=0)[0]
    finally:
        _restore(L)
    rx, ry = np.sqrt(max(x["rr"], 0.0)), np.sqrt(max(y["rr"], 0.0))
    print("2.5nm zero start at 1e-10: sweeps %d (split: %d), true residual %.3e (split: %.3e), f64 rounds %d (split: %d), tile stream %d"
          % (y["iters"], x["iters"], ry, rx, y["f64"], x["f64"], y["stream"]))
    assert y["one"] == 1 and y["products"] == 10 and x["one"] == 0
    assert y["stream"] != 1 and y["f64"] >= 1                                   # no launch streamed an fp32 image
    assert y["width"] == 16 and y["fallback"] == 0 and np.array_equal(x["log"], y["log"])
    assert 0 <= y["rr"] <= p.cg_tol ** 2, y["rr"]
    assert ry <= 2 * rx, (ry, rx)


def _bits(a, b):
    return all(x["iters"] == y["iters"] and x["im"] == y["im"] and x["power"].tobytes() == y["power"].tobytes() for x, y in zip(a, b))


def test_switch(cell_2p5, hip):
    """Form 2 with a pinned degree runs the split form, bit for bit; with the degree from the rule it runs one polynomial; form 0 afterwards restores the
    split form's bits.  (The suite's own defaults pin degree 8: under form 2 every existing test keeps today's path.)"""
    from devicekmc_amd import params as pm
    host, L = hip
    p = pm.KMCParameters(); p.solve_heating_global = True
    try:
        assert L.dkmc_get_x_poly_form() in (0, 1, 2)
        L.dkmc_set_x_poly_form(0); L.dkmc_set_x_poly(8)
        ref = _supersteps(cell_2p5, p, hip, n=2)
        L.dkmc_set_x_poly_form(2)
        assert L.dkmc_get_x_poly_form() == 2
        pinned = _supersteps(cell_2p5, p, hip, n=2)
        L.dkmc_set_x_poly_auto(1)
        ruled = _supersteps(cell_2p5, p, hip, n=2)
        L.dkmc_set_x_poly_form(0); L.dkmc_set_x_poly(8)
        back = _supersteps(cell_2p5, p, hip, n=2)
        L.dkmc_set_x_poly_form(7)                                               # anything else is form 0
        assert L.dkmc_get_x_poly_form() == 0
    finally:
        _restore(L)
    assert all(r["one"] == 0 and r["products"] == 16 for r in ref + pinned + back)
    assert _bits(ref, pinned) and _bits(ref, back)
    assert all(r["one"] == 1 and r["used"] == 8 and r["products"] == N_OF_D[8] for r in ruled), [(r["one"], r["used"], r["products"]) for r in ruled]
    assert all(np.array_equal(a["log"], b["log"]) for a, b in zip(ref, ruled))
