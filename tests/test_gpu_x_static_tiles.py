"""The tunnelling set S with the inner-contact metals first and the all-metal strips of the tile store kept across current solves
(dkmc_set_x_static_tiles; csrc/current.hip step 2, csrc/xt_static.h).  Sizes: 2.5nm -- |S| = 928 with 828 metals (the set as k_atom_rows builds it: the window of the inner
contacts and the dropped ground atom), so 3 strips of 4 can be kept and the fourth mixes metals and vacancies; 7.5nm -- |S| = 8 352.  Every comparison of a partial assembly with a full one is the library's self-check
(dkmc_debug_x_static_verify): the full census and a full fill into buffers of their own, compared word by word with what the assembly left."""
import ctypes as C

import numpy as np
import pytest

from conftest import params_7p5
from test_gpu_parity import Vd, _fresh_device, get, hip  # noqa: F401

pytestmark = pytest.mark.gpu

KEPT, FIRST, METALS, PARAMS, STORE, IMAGE, PREFIX, NOT_APPLICABLE = range(8)        # info[6] of dkmc_get_x_static_info


@pytest.fixture(autouse=True)
def _switches(hip):
    """the tests own the new switches: conftest does not know them"""
    host, L = hip
    L.dkmc_set_x_static_tiles(2); L.dkmc_debug_x_static_verify(0); L.dkmc_set_x_tile_f32(1); L.dkmc_debug_set_x_static_gate(0)
    yield
    L.dkmc_set_x_static_tiles(2); L.dkmc_debug_x_static_verify(0); L.dkmc_set_x_tile_f32(1); L.dkmc_debug_set_x_static_gate(0)


def _workload(name, cell_2p5, dev_7p5):
    from devicekmc_amd import params as pm
    if name == "2.5nm":
        p = pm.KMCParameters()
        s = cell_2p5
    else:
        p = params_7p5()
        s = dev_7p5
    p.solve_heating_global = True
    return s, p


def _info(L):
    from devicekmc_amd.lib import check
    a = (C.c_longlong * 8)(); v = (C.c_longlong * 4)()
    check(L.dkmc_get_x_static_info(a)); check(L.dkmc_debug_get_x_static_verify(v))
    return list(a), list(v)


def _srow(L):
    from devicekmc_amd.lib import check
    n = C.c_int(0)
    check(L.dkmc_xt_get_srow(C.byref(n), None))
    out = np.zeros(n.value, dtype=np.int32)
    check(L.dkmc_xt_get_srow(C.byref(n), out.ctypes.data))
    return out


def _solve(dev, gb, p, V=Vd, k=0):
    dev.updateCharge(gb); dev.updatePotential(gb, p, V, k); dev.updatePower(gb, p, V)


def _superstep(dev, sim, gb, p, k):
    dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, k)
    sim.executeKMCStep(gb, dev, want_log=True)
    dev.updatePower(gb, p, Vd)


def _clean(info, ver):
    return info[7] == 0 and ver == [0, 0, 0, 0]


@pytest.mark.parametrize("which", ["2.5nm", "7.5nm"])
def test_order_of_S(cell_2p5, dev_7p5, hip, which):
    """Mode 0: the system rows of S ascend (atom order, the parent's).  Mode 1: the inner-contact metals first, each group ascending, the same rows."""
    host, L = hip
    s, p = _workload(which, cell_2p5, dev_7p5)
    rows = {}
    for mode in (0, 1):
        L.dkmc_set_x_static_tiles(mode)
        dev, sim, gb, _ = _fresh_device(s, p, hip)
        _solve(dev, gb, p)
        rows[mode] = _srow(L)
        el = get(gb, "atom_element")
        info, _ = _info(L)
        assert info[0] == mode
    r0, r1 = rows[0], rows[1]
    assert np.all(np.diff(r0) > 0)
    metal = np.isin(el[r1 - 2], list(p.metals))
    nM = int(metal.sum())
    assert metal[:nM].all() and not metal[nM:].any()
    assert np.all(np.diff(r1[:nM]) > 0) and np.all(np.diff(r1[nM:]) > 0)
    assert np.array_equal(np.sort(r1), r0)
    assert info[1] == nM // 256 == L.dkmc_x_static_strips(nM)
    print("%s: |S| = %d, %d metals in front" % (which, len(r1), nM))
    assert len(r1) == host.get_stats()["xt_ns"]
    if which == "2.5nm":
        assert (len(r1), nM) == (928, 828)


def test_mode_2_takes_the_new_order_from_its_gate_on(cell_2p5, dev_7p5, hip):
    """The default mode below the measured gate: atom order, nothing kept, "not applicable".  With the gate moved below |S|: the new order, kept strips."""
    host, L = hip
    s, p = _workload("2.5nm", cell_2p5, dev_7p5)
    L.dkmc_debug_x_static_verify(1)
    assert L.dkmc_get_x_static_tiles() == 2
    for gate, order in ((0, 0), (900, 1), (929, 0)):
        L.dkmc_debug_set_x_static_gate(gate)
        dev, sim, gb, _ = _fresh_device(s, p, hip)
        _solve(dev, gb, p); _solve(dev, gb, p, k=1)
        info, ver = _info(L)
        assert info[0] == order and (info[2] > 0) == (order == 1) and info[6] == (KEPT if order else NOT_APPLICABLE), (gate, info)
        assert np.all(np.diff(_srow(L)) > 0) == (order == 0)
        assert ver == [0, 0, 0, 0] and info[7] == (0 if order else -1)


@pytest.mark.parametrize("which", ["2.5nm", "7.5nm"])
def test_partial_assembly_equals_full(cell_2p5, dev_7p5, hip, which):
    """Four coupled supersteps with the self-check on: the first solve keeps nothing (first solve), every later one keeps the all-metal strips, and
    cell masks, fp64 store, fp32 image and X_nnz are those of a full census and a full fill, word for word."""
    host, L = hip
    s, p = _workload(which, cell_2p5, dev_7p5)
    L.dkmc_set_x_static_tiles(1); L.dkmc_debug_x_static_verify(1)
    dev, sim, gb, _ = _fresh_device(s, p, hip)
    for k in range(4):
        _superstep(dev, sim, gb, p, k)
        info, ver = _info(L); st = host.get_stats()
        print("%s step %d: info %s verify %s" % (which, k, info, ver))
        assert info[0] == 1 and info[1] > 0 and _clean(info, ver), (k, info, ver)
        assert info[2] + info[3] == st["spmv_tiles"] and info[4] + info[5] == st["xt_subblocks"]
        if k == 0:
            assert info[2] == 0 and info[4] == 0 and info[6] == FIRST, info
        else:
            assert info[2] > 0 and info[4] > 0 and info[6] == KEPT, info
            assert st["x_tile_stream"] == 1                       # the image's prefix was kept with the store's
    if which == "2.5nm":
        assert info[1] == 3


@pytest.mark.parametrize("extra", [35, 100])
def test_prefix_survives_a_change_of_the_vacancy_count(cell_2p5, dev_7p5, hip, extra):
    """Lattice oxygen turned into vacancies between two solves: +35 takes |S| from 928 to 963 (31 row blocks instead of 29), +100 to 1 028 (5 strips
    instead of 4).  In atom order every tile behind the left contact would move; with the metals first the three all-metal strips are kept."""
    from devicekmc_amd import params as pm
    host, L = hip
    s, p = _workload("2.5nm", cell_2p5, dev_7p5)
    L.dkmc_set_x_static_tiles(1); L.dkmc_debug_x_static_verify(1)
    dev, sim, gb, _ = _fresh_device(s, p, hip)
    _solve(dev, gb, p)
    st = host.get_stats(); info, ver = _info(L)
    assert st["xt_ns"] == 928 and info[6] == FIRST and _clean(info, ver)
    t0, s0 = info[3], info[5]
    el = get(gb, "site_element").copy()
    rng = np.random.default_rng(11)
    el[rng.choice(np.nonzero(el == pm.O_EL)[0], extra, replace=False)] = pm.VACANCY
    gb.t["site_element"].copy_(gb.t["site_element"].new_tensor(el))
    _solve(dev, gb, p, k=1)
    st = host.get_stats(); info, ver = _info(L)
    print("+%d vacancies: info %s verify %s" % (extra, info, ver))
    ns = 928 + extra
    assert st["xt_ns"] == ns and (ns + 31) // 32 == (31 if extra == 35 else 33) and (ns + 255) // 256 == (4 if extra == 35 else 5)
    assert info[1] == 3 and info[2] > 0 and info[4] > 0 and info[6] == KEPT and _clean(info, ver), (info, ver)
    assert info[2] + info[3] > t0 and info[4] + info[5] > s0      # the store grew behind the kept prefix


def test_a_new_bias_point_keeps_nothing(cell_2p5, dev_7p5, hip):
    """Vd 5 -> 4 between two solves moves the metals' CB edges: "metals changed", a full fill, and the prefix is kept again from the solve after."""
    host, L = hip
    s, p = _workload("2.5nm", cell_2p5, dev_7p5)
    L.dkmc_set_x_static_tiles(1); L.dkmc_debug_x_static_verify(1)
    dev, sim, gb, _ = _fresh_device(s, p, hip)
    _solve(dev, gb, p)
    _solve(dev, gb, p, k=1)
    info, ver = _info(L)
    assert info[6] == KEPT and info[2] > 0 and _clean(info, ver)
    dev.setLaplacePotential(gb, p, 4.0)
    _solve(dev, gb, p, V=4.0, k=2)
    info, ver = _info(L)
    assert info[6] == METALS and info[2] == 0 and info[4] == 0 and _clean(info, ver), (info, ver)
    _solve(dev, gb, p, V=4.0, k=3)
    info, ver = _info(L)
    assert info[6] == KEPT and info[2] > 0 and _clean(info, ver), (info, ver)


def test_another_device_keeps_nothing(cell_2p5, dev_7p5, hip):
    """2.5nm, 7.5nm, 2.5nm in one process, the earlier devices still alive: nothing is kept on the first solve of each, the second keeps its prefix."""
    host, L = hip
    L.dkmc_set_x_static_tiles(1); L.dkmc_debug_x_static_verify(1)
    alive = []
    for which in ("2.5nm", "7.5nm", "2.5nm"):
        s, p = _workload(which, cell_2p5, dev_7p5)
        dev, sim, gb, _ = _fresh_device(s, p, hip)
        alive.append((dev, sim, gb))
        _solve(dev, gb, p)
        info, ver = _info(L)
        assert info[2] == 0 and info[4] == 0 and info[6] in (FIRST, METALS) and _clean(info, ver), (which, info, ver)
        _solve(dev, gb, p, k=1)
        info, ver = _info(L)
        assert info[2] > 0 and info[6] == KEPT and _clean(info, ver), (which, info, ver)
    # back on the FIRST device, whose solve is two devices ago: the store holds another device's tiles
    dev, sim, gb = alive[0]
    s, p = _workload("2.5nm", cell_2p5, dev_7p5)
    _solve(dev, gb, p, k=2)
    info, ver = _info(L)
    assert info[2] == 0 and info[6] in (FIRST, METALS) and _clean(info, ver), (info, ver)


def test_the_image_is_not_reused_across_a_toggle(cell_2p5, dev_7p5, hip):
    """dkmc_set_x_tile_f32 toggled between solves: the solve without an image and the first one with an image again fill everything."""
    host, L = hip
    s, p = _workload("7.5nm", cell_2p5, dev_7p5)
    L.dkmc_set_x_static_tiles(1); L.dkmc_debug_x_static_verify(1)
    dev, sim, gb, _ = _fresh_device(s, p, hip)
    want = [(1, FIRST), (1, KEPT), (0, IMAGE), (0, KEPT), (1, IMAGE), (1, KEPT)]
    for k, (f32, reason) in enumerate(want):
        L.dkmc_set_x_tile_f32(f32)
        _solve(dev, gb, p, k=k)
        info, ver = _info(L); st = host.get_stats()
        assert st["x_tile_stream"] == f32
        assert info[6] == reason and (info[2] > 0) == (reason == KEPT) and _clean(info, ver), (k, info, ver)


@pytest.mark.parametrize("which", ["2.5nm", "7.5nm"])
def test_same_operator_in_either_order(cell_2p5, dev_7p5, hip, which):
    """The diagonal pass (T . 1 per system row) under mode 0 and mode 1 on the same state.  The entries of a row of T all have one sign, and the two
    orders are two summation orders of the same ns terms, each within (ns - 1) 2^-53 |d| of the exact sum: |d0 - d1| <= 2 (ns - 1) 2^-53 |d|."""
    from devicekmc_amd.lib import check
    host, L = hip
    s, p = _workload(which, cell_2p5, dev_7p5)
    d = {}
    for mode in (0, 1):
        L.dkmc_set_x_static_tiles(mode)
        dev, sim, gb, _ = _fresh_device(s, p, hip)
        _solve(dev, gb, p)
        st = host.get_stats()
        out = np.zeros(st["N_atom"] + 1)
        check(L.dkmc_xt_get_diag(out.ctypes.data))
        d[mode] = out; ns = st["xt_ns"]; nnz = st["X_nnz"]
        if mode == 0:
            nnz0 = nnz
    assert nnz == nnz0                                           # the same set of entries
    big = np.maximum(np.abs(d[0]), np.abs(d[1]))
    assert np.count_nonzero(d[0]) == ns == np.count_nonzero(d[1]) and np.all(d[0] <= 0) and np.all(d[1] <= 0)
    err = np.abs(d[0] - d[1])
    print("%s: ns %d, max |d0 - d1| / |d| = %.3e (bound %.3e)" % (which, ns, (err[big > 0] / big[big > 0]).max(), 2 * (ns - 1) * 2.0 ** -53))
    assert np.all(err <= 2 * (ns - 1) * 2.0 ** -53 * big)
