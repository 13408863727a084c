"""The preconditioner's N products read a per-solve packed copy of N (dkmc_set_x_nmul_form(1), the default) or the CSR of the neighbour part
(form 0).  Both sum the same products in the same order: the supersteps must agree bit for bit -- sweeps, events, I_macro, T_bg, site power."""
import numpy as np
import pytest

from conftest import params_7p5
from test_gpu_parity import Vd, get, hip  # noqa: F401

pytestmark = pytest.mark.gpu


def _run(structure, hip, form, nsteps):
    host, L = hip
    p = params_7p5(); p.solve_heating_global = True
    dev = host.Device(structure, p)
    sim = host.KMCProcess(dev, p.freq)
    gb = dev.make_gpubuf("cuda:0")
    dev.setLaplacePotential(gb, p, Vd)
    gb.sync_HostToGPU(dev)
    rec = {"iters": [], "log": [], "imacro": [], "T_bg": [], "site_power": []}
    try:
        L.dkmc_set_x_nmul_form(form)
        assert L.dkmc_get_x_nmul_form() == form and L.dkmc_get_x_poly() > 0 and L.dkmc_get_x_block() == 16
        for k in range(nsteps):
            dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, k)
            _, dt = sim.executeKMCStep(gb, dev, want_log=True)
            dev.updatePower(gb, p, Vd)
            rec["iters"].append(host.get_stats()["cg_iters_X"])
            dev.updateTemperature(gb, p, dt)
            rec["log"].append(sim.last_event_log.copy())
            rec["imacro"].append(dev.imacro)
            rec["T_bg"].append(dev.T_bg)
            rec["site_power"].append(get(gb, "site_power").copy())
    finally:
        L.dkmc_set_x_nmul_form(1)
    return rec, (dev, sim, gb)


def test_packed_n_products_bitwise_7p5(dev_7p5, hip):
    """85 071 sites, library defaults (block-CG of width 16, degree-8 preconditioner): three coupled supersteps with the CSR form and the packed
    form of the N products from the same start; both simulations are kept alive so that each keeps its own warm-start state."""
    host, L = hip
    assert L.dkmc_get_x_nmul_form() == 1
    a, keep_a = _run(dev_7p5, hip, 0, 3)
    b, keep_b = _run(dev_7p5, hip, 1, 3)
    print("sweeps per step:", a["iters"], b["iters"])
    assert a["iters"] == b["iters"] and min(a["iters"]) > 0
    for k in range(3):
        assert np.array_equal(a["log"][k], b["log"][k]), k
        assert np.float64(a["imacro"][k]).tobytes() == np.float64(b["imacro"][k]).tobytes(), (k, a["imacro"][k], b["imacro"][k])
        assert np.float64(a["T_bg"][k]).tobytes() == np.float64(b["T_bg"][k]).tobytes(), (k, a["T_bg"][k], b["T_bg"][k])
        assert a["site_power"][k].tobytes() == b["site_power"][k].tobytes(), k
    assert a["imacro"][-1] != 0.0
