"""The packed N products (dkmc_set_x_nmul_form(1)) gathered with 16 bytes per lane (dkmc_set_x_nmul_lane_bytes(16), the default: k_xtb_nmulp16)
against 8 bytes per lane (dkmc_set_x_nmul_lane_bytes(8): k_xtb_nmulp): the same packed N, every output element the same sequence of fp64 operations.
The supersteps must agree bit for bit -- sweeps, events, I_macro, T_bg, site power -- and so must the slab-distributed preconditioned loop on its row
lists (the LIST variant)."""
import numpy as np
import pytest

from conftest import params_7p5
from test_gpu_parity import Vd, get, hip  # noqa: F401

pytestmark = pytest.mark.gpu


def _run(structure, hip, lane_bytes, nsteps):
    host, L = hip
    p = params_7p5(); p.solve_heating_global = True
    dev = host.Device(structure, p)
    sim = host.KMCProcess(dev, p.freq)
    gb = dev.make_gpubuf("cuda:0")
    dev.setLaplacePotential(gb, p, Vd)
    gb.sync_HostToGPU(dev)
    rec = {"iters": [], "log": [], "imacro": [], "T_bg": [], "site_power": []}
    try:
        L.dkmc_set_x_nmul_form(1)
        L.dkmc_set_x_nmul_lane_bytes(lane_bytes)
        assert L.dkmc_get_x_nmul_lane_bytes() == lane_bytes and L.dkmc_get_x_nmul_form() == 1
        assert L.dkmc_get_x_poly() > 0 and L.dkmc_get_x_block() == 16
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
        L.dkmc_set_x_nmul_lane_bytes(16)
    return rec, (dev, sim, gb)


def test_lane_bytes_default_and_setter(hip):
    """16 in a library nobody has set; 8 and 16 are kept as given, anything else selects 16."""
    host, L = hip
    assert L.dkmc_get_x_nmul_lane_bytes() == 16
    try:
        for given, kept in ((8, 8), (16, 16), (0, 16), (4, 16), (32, 16)):
            L.dkmc_set_x_nmul_lane_bytes(given)
            assert L.dkmc_get_x_nmul_lane_bytes() == kept, (given, kept)
    finally:
        L.dkmc_set_x_nmul_lane_bytes(16)


def test_16_byte_n_products_bitwise_7p5(dev_7p5, hip):
    """85 071 sites, library defaults (block-CG of width 16, degree-8 preconditioner): three coupled supersteps with 8 and with 16 bytes per lane
    from the same start; both simulations are kept alive so that each keeps its own warm-start state."""
    a, keep_a = _run(dev_7p5, hip, 8, 3)
    b, keep_b = _run(dev_7p5, hip, 16, 3)
    print("sweeps per step:", a["iters"], b["iters"])
    assert a["iters"] == b["iters"] and min(a["iters"]) > 0
    for k in range(3):
        assert np.array_equal(a["log"][k], b["log"][k]), k
        assert np.float64(a["imacro"][k]).tobytes() == np.float64(b["imacro"][k]).tobytes(), (k, a["imacro"][k], b["imacro"][k])
        assert np.float64(a["T_bg"][k]).tobytes() == np.float64(b["T_bg"][k]).tobytes(), (k, a["T_bg"][k], b["T_bg"][k])
        assert a["site_power"][k].tobytes() == b["site_power"][k].tobytes(), k
    assert a["imacro"][-1] != 0.0


def test_16_byte_n_products_slab_row_lists_same_bits(hip):
    """dkmc_set_x_slab_poly(1), two virtual ranks: the row-list variant with 16 bytes per lane gives the sweeps and the bits of the one with 8.  The
    one-GPU reference of the emulation runs under the same setting, and its two settings agree bit for bit (the test above), so the deviation of the
    distributed solution from it must be the same double."""
    from test_gpu_slab_poly import _emulate, _resident_x
    host, L = hip
    _resident_x()
    out = {}
    try:
        L.dkmc_set_x_slab_poly(1)
        L.dkmc_set_x_nmul_form(1)
        for lane_bytes in (8, 16):
            L.dkmc_set_x_nmul_lane_bytes(lane_bytes)
            out[lane_bytes] = _emulate(L, 2, time_rank=-1)
    finally:
        L.dkmc_set_x_nmul_lane_bytes(16)
        L.dkmc_set_x_slab_poly(0)
    print("lane bytes 8 / 16:", out[8], out[16])
    assert out[8]["sweeps"] == out[16]["sweeps"] > 0 and out[8]["ref"] == out[16]["ref"]
    assert out[8]["rel"] == out[16]["rel"] and 0 <= out[8]["rel"] <= 1e-8
