"""The packed N products with their panel operands served from LDS row windows (dkmc_set_x_nmul_window(1): k_xtb_nmulw; csrc/nwin_plan.h) against the
global gather (0: k_xtb_nmulp16): the same packed N, every output element the same sequence of fp64 operations on the same operands -- so everything
here is compared bit for bit.

a. One Horner step (dkmc_xtb_test_nstep, form 1) over caller-given CSRs of m = 3 ... 2001 rows: bands at +-85 / +-170, a tenth of the columns far
   away, rows wider than 16 and than 32 slots, empty rows, driver columns and the diagonal among the entries; with and without S ranks (the QS-writing
   instantiation); at the default plan, with the cap forced small (a window narrower than a block and a 16-row block with a 16-row halo: both operand
   paths inside one row) and with the cap at zero (every slot gathers from memory).  `out` is pre-filled with NaN.
b. Three coupled supersteps at 2.5 nm and at tile:2 (37 596 sites; its cross-cell neighbours lie outside every window) with the switch at 1 against 0.
c. The default (2: by size) and the values the setter keeps."""
import ctypes as C

import numpy as np
import pytest

from devicekmc_amd.lib import check
from test_gpu_parity import Vd, get, hip  # noqa: F401
from test_gpu_tile_f32 import _workload

pytestmark = pytest.mark.gpu

CAP = 76 * 1024
# (cap bytes, block rows): the default plan; a window narrower than the block; 16-row blocks with a 16-row halo; one row; nothing
PLANS = [(CAP, 320), (CAP, 192), (CAP, 128), (CAP, 256), (40 * 128, 192), (48 * 128, 16), (128, 64), (0, 192)]


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _pattern(m, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(m):
        kind = r % 7
        if 8 <= r < 12 or kind == 6:
            cols = []                                                                       # empty rows (a whole empty slice at rows 8 ... 11)
        else:
            cols = [r + d + j for d in (-170, -85, 85, 170) for j in (-1, 0, 1)]
            if kind == 3:
                cols += list(r - 40 + rng.integers(0, 81, 9))                               # 21 entries: wider than 16 slots
            if kind == 4:
                cols += list(r - 60 + rng.integers(0, 121, 25))                             # 37 entries: wider than 32 slots
            cols = [int(c) if rng.random() >= 0.1 else int(rng.integers(0, m)) for c in cols]      # a tenth anywhere
            cols += [0, 1, r]                                                               # outside N: driver columns, the diagonal
            cols = [c for c in cols if 0 <= c < m]
            cols = [cols[i] for i in rng.permutation(len(cols))]
        rows.append(cols)
    ln = np.array([len(c) for c in rows])
    rp = np.zeros(m + 1, dtype=np.int64); rp[1:] = np.cumsum(ln)
    ci = np.array([c for cols in rows for c in cols], dtype=np.int32)
    nnz = len(ci)
    return rp, ci, rng.uniform(-1.0, 1.0, nnz), rng.uniform(0.5, 2.0, m), rng.standard_normal((m, 16)), rng.standard_normal((m, 16))


def _nstep(L, m, sysm, nsrank, ns):
    rp, ci, val, sc, vin, add = sysm
    out = np.full((m, 16), np.nan)
    qs = np.zeros((max(ns, 1), 16)) if nsrank is not None else None
    check(L.dkmc_xtb_test_nstep(m, _p(rp), _p(ci), _p(val), _p(sc), _p(vin), _p(add), -1.3125, 0.6180339887498949, 1, None, 0, _p(nsrank), ns, _p(out), _p(qs)))
    return out, qs


@pytest.mark.parametrize("m", [3, 5, 17, 63, 191, 193, 577, 2001])
def test_one_step_same_bits(hip, m):
    host, L = hip
    sysm = _pattern(m, seed=m)
    rng = np.random.default_rng(m + 1)
    srows = rng.permutation(np.flatnonzero(rng.random(m) < 0.5))
    nsrank = np.full(m, -1, dtype=np.int32); nsrank[srows] = np.arange(len(srows), dtype=np.int32)
    ns = len(srows)
    try:
        L.dkmc_set_x_nmul_form(1); L.dkmc_set_x_nmul_lane_bytes(16)
        for ranks in ((nsrank, ns), (None, 0)) if ns else ((None, 0),):
            L.dkmc_set_x_nmul_window(0)
            ref, ref_qs = _nstep(L, m, sysm, *ranks)
            assert not np.isnan(ref).any()                                                  # every row is written (rows 0 / 1: ca add)
            L.dkmc_set_x_nmul_window(1)
            for cap, block in PLANS:
                L.dkmc_debug_set_x_nmul_window(cap, block)
                out, qs = _nstep(L, m, sysm, *ranks)
                assert out.tobytes() == ref.tobytes(), (m, cap, block, ranks[1], np.argwhere(out != ref)[:5])
                if ranks[0] is not None:
                    assert qs.tobytes() == ref_qs.tobytes(), (m, cap, block)
    finally:
        L.dkmc_debug_set_x_nmul_window(-1, 0); L.dkmc_set_x_nmul_window(2)


def _run(structure, p, hip, mode, nsteps):
    host, L = hip
    dev = host.Device(structure, p)
    sim = host.KMCProcess(dev, p.freq)
    gb = dev.make_gpubuf("cuda:0")
    dev.setLaplacePotential(gb, p, Vd)
    gb.sync_HostToGPU(dev)
    rec = {"iters": [], "log": [], "imacro": [], "T_bg": [], "site_power": []}
    try:
        L.dkmc_set_x_nmul_window(mode)
        assert L.dkmc_get_x_nmul_window() == mode and L.dkmc_get_x_nmul_form() == 1 and L.dkmc_get_x_nmul_lane_bytes() == 16
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
        L.dkmc_set_x_nmul_window(2)
    return rec, (dev, sim, gb)


@pytest.mark.parametrize("which", ["2.5nm", "tile:2"])
def test_windowed_n_products_bitwise_supersteps(cell_2p5, dev_7p5, hip, which):
    """Three coupled supersteps from the same start with the switch at 0 and at 1; both simulations are kept alive so that each keeps its own
    warm-start state."""
    structure, p = _workload(which, cell_2p5, dev_7p5)
    p.solve_heating_global = True
    a, keep_a = _run(structure, p, hip, 0, 3)
    b, keep_b = _run(structure, p, hip, 1, 3)
    print("sweeps per step:", a["iters"], b["iters"])
    assert a["iters"] == b["iters"] and min(a["iters"]) > 0
    for k in range(3):
        assert np.array_equal(a["log"][k], b["log"][k]), k
        assert np.float64(a["imacro"][k]).tobytes() == np.float64(b["imacro"][k]).tobytes(), (k, a["imacro"][k], b["imacro"][k])
        assert np.float64(a["T_bg"][k]).tobytes() == np.float64(b["T_bg"][k]).tobytes(), (k, a["T_bg"][k], b["T_bg"][k])
        assert a["site_power"][k].tobytes() == b["site_power"][k].tobytes(), k
    assert a["imacro"][-1] != 0.0


def test_window_default_and_setter(hip):
    """2 (by size) in a library nobody has set; 0, 1 and 2 are kept as given, anything else selects 2."""
    host, L = hip
    assert L.dkmc_get_x_nmul_window() == 2
    try:
        for given, kept in ((0, 0), (1, 1), (2, 2), (-1, 2), (3, 2), (16, 2)):
            L.dkmc_set_x_nmul_window(given)
            assert L.dkmc_get_x_nmul_window() == kept, (given, kept)
    finally:
        L.dkmc_set_x_nmul_window(2)
