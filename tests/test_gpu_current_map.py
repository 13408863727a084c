"""The atom-resolved current map (dkmc_set_current_map): through-current, tunnelling share and signed tunnelling outflow per site, computed on
the device from the solved current system, against the host evaluation of the same definitions on the exported X (current_map_ref.py: the
reference and the derived bounds)."""
import ctypes as C

import numpy as np
import pytest

import current_map_ref as cmr
from conftest import params_7p5

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    import __graft_entry__ as g
    g.build()
    from devicekmc_amd import host, lib
    assert torch.cuda.is_available()
    return host, lib.load()


@pytest.fixture(autouse=True)
def _switch_off(hip):
    yield
    hip[1].dkmc_set_current_map(0)


def get(gb, name):
    return gb.t[name].cpu().numpy()


def _solve(hip, structure, p, V, vacancies=0, fmt=1):
    """fresh device -> (300 random vacancies) -> Laplace -> charge -> potential -> power with the switch on"""
    from devicekmc_amd import params as pm
    host, L = hip
    dev = host.Device(structure, p); gb = dev.make_gpubuf("cuda:0")
    if vacancies:
        rng = np.random.default_rng(5)
        el = dev.site_element.copy()
        el[rng.choice(np.nonzero(el == pm.O_EL)[0], vacancies, replace=False)] = pm.VACANCY
        dev.site_element = el
    dev.setLaplacePotential(gb, p, V); gb.sync_HostToGPU(dev)
    dev.updateCharge(gb); dev.updatePotential(gb, p, V, 0)
    L.dkmc_set_x_format(fmt); L.dkmc_set_current_map(1)
    try:
        dev.updatePower(gb, p, V)
    finally:
        L.dkmc_set_x_format(1); L.dkmc_set_current_map(0)
    return dev, gb


def _reference(hip, dev, gb, p):
    host, _ = hip
    X = host.get_last_X()
    m = get(gb, "atom_virtual_potentials")
    return cmr.reference(X, m, get(gb, "atom_x"), get(gb, "atom_y"), get(gb, "atom_z"), cmr.atom_sites(get(gb, "site_element")), dev.N,
                         p.nn_dist, p.lattice, int(p.pbc))


def _check(hip, dev, gb, p):
    ref = _reference(hip, dev, gb, p)
    info = [dev.current_map_info[k] for k in dev.CURRENT_MAP_INFO]
    cmr.check((dev.site_current, dev.site_current_tunnel, dev.site_tunnel_outflow), info, ref, dev.imacro)
    return ref, info


@pytest.mark.parametrize("fmt", [1, 0], ids=["tiled", "csr"])
@pytest.mark.parametrize("V", [5.0, -3.0])
@pytest.mark.parametrize("heating", [False, True])
def test_map_2p5(cell_2p5, hip, heating, V, fmt):
    """2.5 nm cell with 300 extra vacancies, both layouts of X, both signs of the bias, with and without the shift of the heated path: the three
    arrays and info[0 .. 4] within the derived bounds of the host evaluation on the exported X and the potentials left in the buffer; sites
    without a row exactly 0; I_macro the same bits; the signed tunnelling outflow sums to its rounding."""
    from devicekmc_amd import params as pm
    p = pm.KMCParameters(); p.cg_tol = 1e-10; p.solve_heating_global = heating
    dev, gb = _solve(hip, cell_2p5, p, V, vacancies=300, fmt=fmt)
    ref, info = _check(hip, dev, gb, p)
    assert info[6] == (2 if fmt else 0)
    assert ref["thr_tun"].max() > 0 and (ref["thr_all"] > 0).sum() > 0.5 * (dev.N_atom - 1)      # the case has tunnelling current, and current everywhere
    assert abs(info[1]) > 0 and (info[0] > 0) == (V > 0)


@pytest.mark.parametrize("case", ["few_vacancies", "no_vacancies", "empty_S"])
def test_map_edge_cases(cell_2p5, hip, case):
    """Where the tunnelling block degenerates (the recipes of test_tiled_X_edge_cases): very few vacancies, none (S = contact metals only), and an
    empty S -- no tile launch, thr_tun and net_tun all zero, info[6] = 0."""
    from devicekmc_amd import params as pm
    host, L = hip
    p = pm.KMCParameters(); p.solve_heating_global = True; p.cg_tol = 1e-10
    p.initial_vacancy_concentration = 0.002 if case == "few_vacancies" else 0.0
    if case == "empty_S":
        p.num_layers_contact = 100
    dev, gb = _solve(hip, cell_2p5, p, 5.0)
    ref, info = _check(hip, dev, gb, p)
    if host.get_stats()["xt_ns"] == 0:
        assert case == "empty_S"
        assert not dev.site_current_tunnel.any() and not dev.site_tunnel_outflow.any() and info[6] == 0 and info[4] == 0.0
    else:
        assert case != "empty_S" and info[6] == 2


def test_map_7p5_and_plane_profile(dev_7p5, hip):
    """85 071 sites: multi-strip runs, records shared by four waves, a padded S and partial tiles.  The map within the bounds, and the tunnelling
    current crossing three planes inside the oxide (Device.tunnel_current_profile) against the host sum of the classified entries that cross."""
    p = params_7p5(); p.solve_heating_global = True
    dev, gb = _solve(hip, dev_7p5, p, 5.0)
    ref, info = _check(hip, dev, gb, p)
    assert info[6] == 2 and ref["thr_tun"].max() > 0
    from devicekmc_amd import params as pm
    x, el = np.asarray(dev.site_x), get(gb, "site_element")
    ox = x[(el == pm.O_EL) | (el == pm.VACANCY)]
    cuts = [float(ox.min() + f * (ox.max() - ox.min())) for f in (0.25, 0.5, 0.75)]
    got = dev.tunnel_current_profile(cuts)
    for g, (h, b) in zip(got, cmr.profile_reference(ref, x, cuts)):
        assert abs(g - h) <= b, (g, h, b)
    assert max(abs(g) for g in got) > 0


def _trajectory(hip, structure, switch, nsteps=2):
    """nsteps supersteps of a fresh device with the switch set; everything a caller can observe of them"""
    from devicekmc_amd import params as pm
    host, L = hip
    V = 5.0
    p = pm.KMCParameters(); p.solve_heating_global = True
    dev = host.Device(structure, p); sim = host.KMCProcess(dev, p.freq); gb = dev.make_gpubuf("cuda:0")
    dev.setLaplacePotential(gb, p, V); gb.sync_HostToGPU(dev)
    L.dkmc_set_current_map(switch)
    rec = []
    for k in range(nsteps):
        dev.updateCharge(gb); dev.updatePotential(gb, p, V, k)
        _, dt = sim.executeKMCStep(gb, dev, want_log=True)
        dev.updatePower(gb, p, V); dev.updateTemperature(gb, p, dt)
        n = C.c_int(0)
        assert L.dkmc_get_current_warm_vector(C.byref(gb.c), None, 0, C.byref(n)) == 0
        warm = np.zeros(n.value)
        assert L.dkmc_get_current_warm_vector(C.byref(gb.c), warm.ctypes.data_as(C.c_void_p), n.value, C.byref(n)) == 0
        st = host.get_stats()
        step = dict(m=get(gb, "atom_virtual_potentials").copy(), imacro=dev.imacro, power=get(gb, "site_power").copy(),
                    log=np.array(sim.last_event_log).copy(), warm=warm, iters=st["cg_iters_X"], nnz=st["X_nnz"], dt=dt)
        if switch:
            step["map"] = (dev.site_current.copy(), dev.site_current_tunnel.copy(), dev.site_tunnel_outflow.copy(), dict(dev.current_map_info))
        rec.append(step)
    L.dkmc_set_current_map(0)
    return rec


def test_switch_is_neutral_and_the_map_deterministic(cell_2p5, hip):
    """Two supersteps with the switch on against the same two of a fresh device with it off: potentials, I_macro, dissipated power, event log and
    the warm-start vector bit for bit.  Two runs with the switch on give the same bits of the map; a run after the switch went off again has the
    solver statistics of one that never saw it."""
    off, on1, on2, off2 = (_trajectory(hip, cell_2p5, s) for s in (0, 1, 1, 0))
    for a, b, c, d in zip(off, on1, on2, off2):
        for other in (b, c, d):
            for k in ("m", "power", "log", "warm"):
                assert np.array_equal(a[k], other[k]), k
            assert a["imacro"] == other["imacro"] and a["dt"] == other["dt"]
        for u, v in zip(b["map"][:3], c["map"][:3]):
            assert u.tobytes() == v.tobytes()
        assert b["map"][3] == c["map"][3] and b["map"][0].max() > 0
        assert (a["iters"], a["nnz"]) == (d["iters"], d["nnz"])


def test_two_buffers_keep_their_own_map(cell_2p5, hip):
    """Two GPUBuffers in one process at different biases, solved alternately: each returns its own map (the bits of a run that has the device
    alone).  A buffer that never solved with the switch on reports an error that names the call, and the library goes on after dkmc_clear_error."""
    from devicekmc_amd import params as pm
    host, L = hip
    pa = pm.KMCParameters(); pa.solve_heating_global = True
    pb = pm.KMCParameters(); pb.solve_heating_global = True; pb.rnd_seed = 7

    def make(p, V):
        dev = host.Device(cell_2p5, p); gb = dev.make_gpubuf("cuda:0")
        dev.setLaplacePotential(gb, p, V); gb.sync_HostToGPU(dev)
        dev.updateCharge(gb); dev.updatePotential(gb, p, V, 0)
        return dev, gb

    def fetch(dev, gb):
        out = [np.empty(dev.N) for _ in range(3)]
        assert L.dkmc_copy_current_map_from_gpu(C.byref(gb.c), *[o.ctypes.data_as(C.c_void_p) for o in out]) == 0
        info = (C.c_double * 8)()
        assert L.dkmc_get_current_map_info(C.byref(gb.c), info) == 0
        return [o.tobytes() for o in out] + [list(info)]

    alone = []
    for p, V in ((pa, 5.0), (pb, 3.0)):
        dev, gb = make(p, V)
        L.dkmc_set_current_map(1)
        dev.updatePower(gb, p, V)
        alone.append(fetch(dev, gb))
        L.dkmc_set_current_map(0)
        del dev, gb
    (da, ga), (db, gb_), (dc, gc) = make(pa, 5.0), make(pb, 3.0), make(pa, 5.0)
    L.dkmc_set_current_map(1)
    da.updatePower(ga, pa, 5.0); db.updatePower(gb_, pb, 3.0)
    L.dkmc_set_current_map(0)
    dc.updatePower(gc, pa, 5.0)                                   # solved, but never with the switch on
    assert fetch(db, gb_) == alone[1] and fetch(da, ga) == alone[0] and alone[0][0] != alone[1][0]
    assert fetch(da, ga)[3][0] == da.imacro and fetch(db, gb_)[3][0] == db.imacro
    buf = np.empty(dc.N)
    for call in ("dkmc_copy_current_map_from_gpu", "dkmc_get_current_map_info"):
        if call == "dkmc_copy_current_map_from_gpu":
            rc = L.dkmc_copy_current_map_from_gpu(C.byref(gc.c), buf.ctypes.data_as(C.c_void_p), None, None)
        else:
            rc = L.dkmc_get_current_map_info(C.byref(gc.c), (C.c_double * 8)())
        assert rc != 0 and call in L.dkmc_last_error().decode() and "dkmc_set_current_map" in L.dkmc_last_error().decode()
        L.dkmc_clear_error()
        assert L.dkmc_last_error().decode() == ""
    # NULL pointers are skipped, and the library carries on
    one = np.empty(da.N)
    assert L.dkmc_copy_current_map_from_gpu(C.byref(ga.c), None, None, one.ctypes.data_as(C.c_void_p)) == 0
    assert one.tobytes() == alone[0][2]
    dc.updatePower(gc, pa, 5.0)
    assert abs(dc.imacro / da.imacro - 1) <= 1e-4
