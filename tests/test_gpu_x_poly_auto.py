"""The degree rule of the split polynomial preconditioner (dkmc_set_x_poly_auto; csrc/xtb_precond.h: xtb_poly_rule): with the breakpoints moved
(dkmc_set_x_poly_auto_rows) a small system falls into every branch in turn -- the solve runs the branch's degree and gives the supersteps of the pinned
degree 8 --, and dkmc_set_x_poly pins a degree or turns the preconditioner off whatever the rule says."""
import numpy as np
import pytest

from test_gpu_parity import Vd, _fresh_device, get, hip  # noqa: F401
from test_gpu_tile_f32 import _workload

pytestmark = pytest.mark.gpu

# I_macro between the block loop at two degrees of the preconditioner at the default tolerance: the bound of
# tests/test_gpu_block_cg.py::test_split_polynomial_preconditioner_7p5 (`ibound` at 1e-6), used for site_power (against its largest entry) as well
REL_BETWEEN_DEGREES = 1e-5


BIG = 1 << 30       # rows no system here reaches


def _branches(L, m):
    """per branch of the rule: breakpoints that put a system of m rows into it, and the branch's degree"""
    out = []
    for n0, n1 in ((BIG, BIG + 1), (1, BIG), (1, 2)):
        L.dkmc_set_x_poly_auto_rows(n0, n1)
        out.append((n0, n1, L.dkmc_xtb_poly_rule(m)))
    L.dkmc_set_x_poly_auto_rows(0, 0)
    assert out[0][2] == L.dkmc_xtb_poly_rule(3) and out[2][2] == L.dkmc_xtb_poly_rule(BIG)       # first and last step of the measured rule
    return out


def _supersteps(structure, p, hip, n=3):
    """one cold and n - 1 warm coupled supersteps: event logs, I_macro, site power and the stats of every step"""
    host, L = hip
    dev, sim, gb, _ = _fresh_device(structure, p, hip)
    rec = []
    for k in range(n):
        dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, k)
        sim.executeKMCStep(gb, dev, want_log=True)
        dev.updatePower(gb, p, Vd)
        st = host.get_stats()
        rec.append(dict(log=np.array(sim.last_event_log).copy(), im=dev.imacro, power=get(gb, "site_power").copy(), iters=st["cg_iters_X"], rr=st["cg_rr_X"],
                        used=st["xb_poly_used"], width=st["xb_width"], fallback=st["xb_fallback"], rows=st["N_atom"] + 1))
    return rec


@pytest.mark.parametrize("which", ["2.5nm", "tile:2"])
def test_every_branch_of_the_rule_gives_the_supersteps_of_degree_8(cell_2p5, dev_7p5, hip, which):
    host, L = hip
    structure, p = _workload(which, cell_2p5, dev_7p5)
    p.solve_heating_global = True
    try:
        L.dkmc_set_x_poly(8)
        assert L.dkmc_get_x_poly_auto() == 0 and L.dkmc_get_x_poly() == 8
        ref = _supersteps(structure, p, hip)
        assert all(r["used"] == 8 and r["width"] == 16 and not r["fallback"] for r in ref)
        m = ref[0]["rows"]
        branches = _branches(L, m)
        L.dkmc_set_x_poly_auto(1)
        assert L.dkmc_get_x_poly_auto() == 1 and L.dkmc_get_x_poly() == 8          # (the base degree stays what it was)
        for n0, n1, degree in branches:
            assert 1 <= degree <= 16
            L.dkmc_set_x_poly_auto_rows(n0, n1)
            got = _supersteps(structure, p, hip)
            for k, (x, y) in enumerate(zip(ref, got)):
                di = abs(y["im"] / x["im"] - 1); dp = np.abs(y["power"] - x["power"]).max() / np.abs(x["power"]).max()
                print("%s branch (%d, %d) degree %d step %d: sweeps %d (degree 8: %d), true residual %.3e, rel dI_macro %.3e, rel dpower %.3e"
                      % (which, n0, n1, degree, k, y["iters"], x["iters"], np.sqrt(max(y["rr"], 0.0)), di, dp))
                assert y["used"] == degree, (k, y["used"], degree)
                assert y["width"] == 16 and y["fallback"] == 0
                assert y["rr"] <= p.cg_tol ** 2, (k, y["rr"])
                assert np.array_equal(x["log"], y["log"]), (degree, k)
                assert di <= REL_BETWEEN_DEGREES and dp <= REL_BETWEEN_DEGREES, (degree, k, di, dp)
    finally:
        L.dkmc_set_x_poly_auto_rows(0, 0); L.dkmc_set_x_poly(8)


def test_an_explicit_degree_pins_it_and_zero_turns_the_preconditioner_off(cell_2p5, dev_7p5, hip):
    host, L = hip
    structure, p = _workload("2.5nm", cell_2p5, dev_7p5)
    p.solve_heating_global = True
    try:
        L.dkmc_set_x_poly_auto(1)
        ruled = _supersteps(structure, p, hip, n=1)[0]
        assert ruled["used"] == L.dkmc_xtb_poly_rule(ruled["rows"]) > 0
        m = ruled["rows"]
        for n0, n1 in ((0, 0), (BIG, BIG + 1), (1, 2)):
            L.dkmc_set_x_poly(4)                                                     # pins 4 and clears the rule, whatever the breakpoints
            L.dkmc_set_x_poly_auto_rows(n0, n1)
            assert L.dkmc_get_x_poly_auto() == 0 and L.dkmc_get_x_poly() == 4
            a = _supersteps(structure, p, hip, n=1)[0]
            assert a["used"] == 4 and a["width"] == 16 and not a["fallback"]
        L.dkmc_set_x_poly_auto_rows(0, 0)
        L.dkmc_set_x_poly(0)
        assert L.dkmc_get_x_poly_auto() == 0 and L.dkmc_get_x_poly() == 0
        plain = _supersteps(structure, p, hip, n=1)[0]
        assert plain["used"] == 0 and plain["width"] == 16 and not plain["fallback"]
        assert host.get_stats()["x_tile_stream"] == 0                              # the plain loop: fp64 store
        assert plain["iters"] > ruled["iters"]
        L.dkmc_set_x_poly_auto(1)                                                  # the rule is back (the base degree returns from 0 to the default)
        assert L.dkmc_get_x_poly_auto() == 1 and L.dkmc_get_x_poly() == 8
        back = _supersteps(structure, p, hip, n=1)[0]
        assert back["used"] == ruled["used"] and back["width"] == 16 and not back["fallback"]
        assert np.array_equal(back["log"], ruled["log"])
    finally:
        L.dkmc_set_x_poly_auto_rows(0, 0); L.dkmc_set_x_poly(8)
