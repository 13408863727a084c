"""The filament analysis on the device (dkmc_find_clusters, csrc/clusters.hip) against the host reference cluster_ref.py: labels, component table
and info -- the doubles included -- with np.array_equal; the number of labelling rounds against the reference's synchronous model."""
import ctypes as C

import numpy as np
import pytest

import cluster_ref as cr
from analysis_support import _chain, _dev, hip  # noqa: F401
from conftest import params_7p5

pytestmark = pytest.mark.gpu

BOTH = cr.METAL | cr.VACANCY_BIT


@pytest.fixture(autouse=True)
def _default_cap(hip):
    yield
    hip[1].dkmc_debug_set_cluster_round_cap(0)


def run_raw(hip, index, element, charge, x, metals, members, n_left, n_right, capacity=None):
    """the raw entry point on host arrays -> (labels as a host array, table, info)"""
    host, _ = hip
    index = np.asarray(index)
    label, table, info = host.find_clusters(_dev(index, np.int32), index.shape[1], _dev(element, np.int32),
                                            None if charge is None else _dev(charge, np.int32), _dev(x, np.float64), _dev(metals, np.int32),
                                            members, n_left, n_right, capacity)
    return label.cpu().numpy(), table, info


def check_raw(hip, index, element, charge, x, metals, members, n_left, n_right):
    ref = cr.analyse(index, element, charge, x, metals, members, n_left, n_right)
    got = run_raw(hip, index, element, charge, x, metals, members, n_left, n_right)
    cr.assert_equal(*got, ref)
    return got, ref


# ---- the golden devices ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev_2p5(hip, cell_2p5):
    from devicekmc_amd import params as pm
    host, _ = hip
    p = pm.KMCParameters()
    dev = host.Device(cell_2p5, p)
    return dev, dev.make_gpubuf("cuda:0"), p, dev.site_element.copy()


def _device_ref(dev, gb, p, members, index=None):
    el, ch = gb.t["site_element"].cpu().numpy(), gb.t["site_charge"].cpu().numpy()
    nl, nr = dev.get_num_in_contacts(p.num_atoms_first_layer, "left"), dev.get_num_in_contacts(p.num_atoms_first_layer, "right")
    return cr.analyse(dev.neigh_idx if index is None else index, el, ch, dev.site_x, list(p.metals), members, nl, nr)


@pytest.mark.parametrize("members", [BOTH, cr.VACANCY_BIT, cr.VACANCY_BIT | cr.NEUTRAL_ONLY], ids=["metal+vacancy", "vacancy", "neutral-vacancy"])
def test_device_2p5(hip, dev_2p5, members):
    dev, gb, p, _ = dev_2p5
    if members & cr.NEUTRAL_ONLY:
        dev.updateCharge(gb)
        ch, el = gb.t["site_charge"].cpu().numpy(), gb.t["site_element"].cpu().numpy()
        assert int((ch[el == 2] != 0).sum()) > 0                                  # some vacancies are charged
    ref = _device_ref(dev, gb, p, members)
    label, table, info = dev.find_clusters(gb, members=members)
    cr.assert_equal(label, table, info, ref)
    assert dev.site_cluster is label and dev.cluster_info is info and dev.cluster_table is table
    if members == BOTH:
        assert (info["n_members"], info["n_components"]) == (3521, 79)
    if members == cr.VACANCY_BIT:
        assert (info["n_members"], info["n_components"]) == (100, 83)


@pytest.mark.parametrize("r,skip,components,bridged", [(3.0, None, 65, 1), (3.0, (25.0, 40.0), 70, 0), (2.0, None, 73, 0)])
def test_planted_filament_2p5(hip, dev_2p5, r, skip, components, bridged):
    """the bridged flag flips with the planted filament; tips and gap are the numpy values bit for bit"""
    import torch
    dev, gb, p, el0 = dev_2p5
    el2, _ = cr.plant_filament(el0, dev.site_x, dev.site_y, dev.site_z, r, skip)
    try:
        dev.site_element = el2
        gb.t["site_element"].copy_(torch.as_tensor(el2))
        ref = _device_ref(dev, gb, p, BOTH)
        label, table, info = dev.find_clusters(gb)
        cr.assert_equal(label, table, info, ref)
        assert info["n_components"] == components and info["bridged"] == bridged
        assert info["bridge_root"] == (0 if bridged else -1) and (info["gap_x"] == 0.0) == bool(bridged)
    finally:
        dev.site_element = el0.copy()
        gb.t["site_element"].copy_(torch.as_tensor(el0))


def test_wide_index_2p5(hip, dev_2p5):
    """an index of several hundred entries per row (7.0 A): nothing assumes nn <= 64"""
    import torch
    host, _ = hip
    dev, gb, p, _ = dev_2p5
    wide, nn = host.build_neighbor_index_gpu(dev.site_x, dev.site_y, dev.site_z, p.lattice, p.pbc, 7.0)
    assert nn > 128
    ref = _device_ref(dev, gb, p, cr.VACANCY_BIT, index=wide)
    label, table, info = dev.find_clusters(gb, members=host.VACANCY, link_index=(torch.as_tensor(wide.reshape(-1)).to("cuda:0"), nn))
    cr.assert_equal(label, table, info, ref)
    assert info["n_components"] <= 83                                       # the wider links merge clusters of the nearest-neighbour index


def test_device_7p5(hip, dev_7p5):
    host, _ = hip
    p = params_7p5()
    dev = host.Device(dev_7p5, p, gpu_neighbors="cuda:0")
    gb = dev.make_gpubuf("cuda:0")
    ref = _device_ref(dev, gb, p, BOTH)
    label, table, info = dev.find_clusters(gb)
    cr.assert_equal(label, table, info, ref)
    assert (info["n_members"], info["n_components"]) == (31681, 629)


# ---- synthetic indices through the raw entry point ----------------------------------------------------------------------------------------
def _chain(n, scrambled, seed=3):
    order = np.random.default_rng(seed).permutation(n) if scrambled else np.arange(n)
    index = np.full((n, 2), -1, dtype=np.int32)
    index[order[:-1], 0] = order[1:]; index[order[1:], 1] = order[:-1]
    return index


@pytest.fixture(scope="module")
def scrambled_chain():
    n = 200000
    rng = np.random.default_rng(11)
    return _chain(n, True), np.full(n, 2, dtype=np.int32), rng.normal(size=n)


def test_scrambled_chain(hip, scrambled_chain):
    index, element, x = scrambled_chain
    (label, table, info), _ = check_raw(hip, index, element, None, x, [6], cr.VACANCY_BIT, 10, 10)
    assert not label.any() and info["n_components"] == 1 and table["size"][0] == len(element) and info["bridged"] == 1
    assert 3 <= info["rounds"] < 64


def test_ordered_chain(hip):
    n = 200000
    (label, _, info), _ = check_raw(hip, _chain(n, False), np.full(n, 2, dtype=np.int32), None, np.linspace(-3.0, 7.0, n), [6], cr.VACANCY_BIT, 1, 1)
    assert not label.any() and info["rounds"] == 2


def test_star(hip):
    n, centre = 257, 100
    index = np.full((n, n - 1), -1, dtype=np.int32)
    index[centre] = np.delete(np.arange(n), centre)
    (label, _, info), _ = check_raw(hip, index, np.full(n, 6, dtype=np.int32), None, np.cos(np.arange(n)), [6], cr.METAL, 0, 0)
    assert not label.any() and info["largest_free_size"] == n


def _random_graph(rng, N, nn, one_way):
    index = rng.integers(0, N, size=(N, nn)).astype(np.int32)
    index[rng.random((N, nn)) < 0.4] = -1                                         # padding anywhere in a row
    if one_way:
        index[(index >= 0) & (index < np.arange(N)[:, None])] = -1
    element = rng.choice([2, 3, 6], N, p=[0.35, 0.3, 0.35]).astype(np.int32)
    return index, element, (rng.integers(0, 2, N) * 2).astype(np.int32), rng.normal(size=N) * 5.0


@pytest.mark.parametrize("one_way", [False, True], ids=["both-ways", "one-way"])
@pytest.mark.parametrize("N,nn", [(1, 1), (63, 2), (65, 3), (257, 2), (5000, 3), (3000, 130)])
def test_random_graphs(hip, N, nn, one_way):
    """padding in mid-row, one-directional entries, sizes around the wave and the workgroup, both lane layouts of the row pass"""
    rng = np.random.default_rng(7 * N + nn + one_way)
    index, element, charge, x = _random_graph(rng, N, nn, one_way)
    if nn == 130:
        index[rng.random(index.shape) < 0.985] = -1                                # keep the graph sparse enough to have many components
    for members in (BOTH, cr.VACANCY_BIT | cr.NEUTRAL_ONLY):
        check_raw(hip, index, element, charge, x, [6, 7], members, N // 5, N // 3)


def test_degenerate_member_sets(hip):
    N = 300
    rng = np.random.default_rng(2)
    index, _, _, x = _random_graph(rng, N, 4, False)
    # no member at all: no components, no error
    (label, table, info), _ = check_raw(hip, index, np.full(N, 3, dtype=np.int32), None, x, [6], BOTH, 50, 50)
    assert (label == -1).all() and info["n_components"] == 0 and info["n_members"] == 0 and len(table["root"]) == 0 and info["rounds"] == 1
    assert info["bridge_root"] == -1 and info["tip_left_x"] == -np.inf and info["tip_right_x"] == np.inf and info["gap_x"] == np.inf
    # one member
    el = np.full(N, 3, dtype=np.int32); el[123] = 2
    (label, table, info), _ = check_raw(hip, index, el, None, x, [6], BOTH, 50, 50)
    assert info["n_components"] == 1 and table["root"][0] == 123 and table["xmin"][0] == x[123] == table["xmax"][0] and table["flags"][0] == 0
    # N isolated members
    (label, table, info), _ = check_raw(hip, np.full((N, 3), -1, dtype=np.int32), np.full(N, 6, dtype=np.int32), None, x, [6], BOTH, 50, 50)
    assert np.array_equal(label, np.arange(N)) and info["n_components"] == N and np.array_equal(table["xmin"], x)


def test_table_capacity(hip):
    rng = np.random.default_rng(5)
    index, element, charge, x = _random_graph(rng, 2000, 2, False)
    ref = cr.analyse(index, element, charge, x, [6], BOTH, 100, 100)
    assert ref[2]["n_components"] > 40
    label, table, info = run_raw(hip, index, element, charge, x, [6], BOTH, 100, 100, capacity=40)
    assert len(table["root"]) == 40 and info["n_components"] == ref[2]["n_components"]      # the first rows, and the true count
    cr.assert_equal(label, table, info, ref, rows=40)
    label, table, info = run_raw(hip, index, element, charge, x, [6], BOTH, 100, 100, capacity=0)
    assert len(table["root"]) == 0 and info["n_components"] == ref[2]["n_components"]


def test_round_cap(hip, scrambled_chain):
    """a labelling that is not finished at the cap is an error return with a message, never labels; the next call under the default cap succeeds"""
    import torch
    host, L = hip
    index, element, x = scrambled_chain
    n = len(element)
    ti, te, tx, tm = _dev(index, np.int32), _dev(element, np.int32), _dev(x, np.float64), _dev([6], np.int32)
    label = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    host._use_stream(label.device)
    L.dkmc_debug_set_cluster_round_cap(1)
    args = (n, 2, host._ptr(ti), host._ptr(te), None, host._ptr(tx), host._ptr(tm), 1, cr.VACANCY_BIT, 10, 10, host._ptr(label))
    rc = L.dkmc_find_clusters(*args)
    msg = L.dkmc_last_error().decode()
    L.dkmc_clear_error()
    assert rc != 0 and "dkmc_find_clusters" in msg and "1 rounds" in msg
    assert (label.cpu().numpy() == -1).all()
    i8, x3 = (C.c_int * 8)(), (C.c_double * 3)()
    assert L.dkmc_get_cluster_info(i8, x3) != 0                                   # no info of a failed call
    L.dkmc_clear_error()
    L.dkmc_debug_set_cluster_round_cap(0)
    assert L.dkmc_find_clusters(*args) == 0 and L.dkmc_get_cluster_info(i8, x3) == 0
    assert not label.cpu().numpy().any() and i8[1] == 1 and 3 <= i8[5] < 64


# ---- purity ----------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_same_bytes(hip):
    rng = np.random.default_rng(9)
    index, element, charge, x = _random_graph(rng, 20000, 6, False)
    a = run_raw(hip, index, element, charge, x, [6], BOTH, 500, 500)
    b = run_raw(hip, index, element, charge, x, [6], BOTH, 500, 500)
    assert a[0].tobytes() == b[0].tobytes() and a[2] == b[2]
    for k in cr.TABLE:
        assert a[1][k].tobytes() == b[1][k].tobytes(), k


def _supersteps(hip, structure, analyse):
    """three coupled supersteps at 5 V; analyse: the analysis is called between every two phases.  Returns what a run must reproduce bit for bit."""
    from devicekmc_amd import params as pm
    host, L = hip
    p = pm.KMCParameters(); p.solve_heating_global = True
    dev = host.Device(structure, p); sim = host.KMCProcess(dev, p.freq); gb = dev.make_gpubuf("cuda:0")
    dev.setLaplacePotential(gb, p, 5.0); gb.sync_HostToGPU(dev)
    out = []

    def look():
        if analyse:
            dev.find_clusters(gb)
            dev.find_clusters(gb, members=host.VACANCY | host.NEUTRAL_ONLY)

    for step in range(3):
        look(); dev.updateCharge(gb)
        look(); dev.updatePotential(gb, p, 5.0, step)
        look(); _, dt = sim.executeKMCStep(gb, dev, want_log=True)
        look(); dev.updatePower(gb, p, 5.0)
        look(); dev.updateTemperature(gb, p, dt)
        look()
        n = C.c_int(0)
        host.check(L.dkmc_get_current_warm_vector(C.byref(gb.c), None, 0, C.byref(n)))
        warm = np.zeros(n.value)
        host.check(L.dkmc_get_current_warm_vector(C.byref(gb.c), host._np_ptr(warm), n.value, C.byref(n)))
        out.append(dict(log=sim.last_event_log.copy(), dt=dt, imacro=dev.imacro, T_bg=dev.T_bg, warm=warm,
                        **{k: gb.t[k].cpu().numpy() for k in ("site_element", "site_charge", "site_potential_boundary", "site_potential_charge",
                                                              "site_power", "atom_virtual_potentials")}))
    return out


def test_supersteps_unchanged_by_the_analysis(hip, cell_2p5):
    plain, watched = _supersteps(hip, cell_2p5, False), _supersteps(hip, cell_2p5, True)
    for a, b in zip(plain, watched):
        assert len(a["log"]) > 0 and a["warm"].size > 0
        for k in a:
            va, vb = np.asarray(a[k]), np.asarray(b[k])
            assert va.dtype == vb.dtype and va.tobytes() == vb.tobytes(), k
