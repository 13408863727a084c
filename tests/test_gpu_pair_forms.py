"""The queued form of the pair sum's kernels (dkmc_set_pair_form(1), csrc/potential.hip: pw_sweep<1> / pw_drain) against form 0.  Form 1 tests a pair
as form 0 does, queues the passing ones per wave in LDS and evaluates 64 of them at a time; it keeps form 0's eight class sums per site, adds the
terms to each in list order and combines them the same way, so every potential must keep its BITS -- and the two counters of dkmc_stats their
values.  Shapes: the 2.5 nm cell (9 399 sites = 146 x 64 + 55: k_pairwise with a partial last workgroup, lists of 0, 3 and ~750 charged sites),
tile:4 (150 384 sites: the smallest tile:K whose box gives the cell list, 6 x 6 columns of which a chunk sweeps up to 25, more than one LDS tile,
so the queue carries across tiles), and three coupled supersteps of 7.5nm and tile:4.  conftest.py does not know the switch: every test restores
form 0, the cut-off and profiling in a `finally`."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_kcg_windows import Vd, _fresh
from test_gpu_parity import get, make_pair, put

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__ as g
    g.build()
    from devicekmc_amd import host, lib
    return host, lib.load()


def _restore(L):
    L.dkmc_set_pair_form(0); L.dkmc_set_pair_cutoff(6.5); L.dkmc_set_profiling(0)


def _info(L):
    from devicekmc_amd import lib
    info, ms = (C.c_longlong * 6)(), (C.c_double * 2)()
    lib.check(L.dkmc_get_pair_sum_info(info, ms))
    return list(info), list(ms)


def _sum(hip, gb, pbc, form, cut):
    """One profiled pair sum: (potentials, pair_evaluated, pair_tested, info[6]).  The caller restores the switches."""
    from devicekmc_amd.host import _ptr
    from devicekmc_amd.lib import check
    host, L = hip
    L.dkmc_set_pair_form(form); L.dkmc_set_pair_cutoff(cut); L.dkmc_set_profiling(1)
    assert L.dkmc_get_pair_form() == form
    check(L.dkmc_poisson_gridless_gpu(0, int(pbc), gb.N_, _ptr(gb.lattice), _ptr(gb.sigma), _ptr(gb.k), _ptr(gb.site_x), _ptr(gb.site_y),
                                      _ptr(gb.site_z), _ptr(gb.site_charge), _ptr(gb.site_potential_charge)))
    st = host.get_stats()
    info, ms = _info(L)
    assert ms[0] == st["pair_ms"] and 0.0 < ms[1] <= ms[0]
    return get(gb, "site_potential_charge").copy(), st["pair_evaluated"], st["pair_tested"], info


def _oracle_sum(N, x, y, z, lattice, pbc, p, q):
    from oracle import oracle as oc
    want = np.zeros(N)
    lat = np.asarray(lattice, dtype=np.float64)
    oc.lib().okmc_poisson_gridless(N, oc._p(x), oc._p(y), oc._p(z), oc._p(lat), int(pbc), C.c_double(p.sigma), C.c_double(p.k), oc._p(q), oc._p(want))
    return want


def _dense(info, evaluated):
    """The queue was taken and is dense: every wave (4 per workgroup) wastes at most one partial batch of at most 63 empty slots."""
    assert info[4] >= evaluated and info[4] % 64 == 0
    assert info[4] - evaluated <= 63 * 4 * info[2], (info, evaluated)


@pytest.fixture(scope="module")
def small(cell_2p5, hip):
    from devicekmc_amd import params as pm
    p = pm.KMCParameters()
    dev, sim, gb, o = make_pair(cell_2p5, p, hip)
    assert dev.N == 9399 and dev.N % 64 == 55
    rng = np.random.default_rng(11)
    q = np.where(rng.random(dev.N) < 0.08, rng.choice([-2, 2], dev.N), 0).astype(np.int32)          # test_pair_sum_all_pairs_switch's charges
    q3 = np.zeros(dev.N, dtype=np.int32); q3[[5, 4000, dev.N - 1]] = [2, -2, 2]                     # entries for waves 0-2 only; no batch fills
    charges = {"random": q, "three": q3, "none": np.zeros(dev.N, dtype=np.int32)}
    want = {(name, pbc): _oracle_sum(dev.N, dev.site_x, dev.site_y, dev.site_z, p.lattice, pbc, p, qq) for name, qq in charges.items() for pbc in (0, 1)}
    return p, dev, gb, charges, want


@pytest.mark.parametrize("pbc", [0, 1])
@pytest.mark.parametrize("name", ["random", "three", "none"])
def test_k_pairwise_same_bits(small, hip, name, pbc):
    """k_pairwise at its smallest shape, cut-off 6.5 and 0 (all pairs): form 1 against form 0 bit for bit with equal counters, against the oracle to
    1e-12 of the largest potential (test_pair_sum_all_pairs_switch's bound)."""
    host, L = hip
    p, dev, gb, charges, want = small
    q, w = charges[name], want[(name, pbc)]
    nq = int((q != 0).sum())
    put(gb, "site_charge", q)
    try:
        for cut in (6.5, 0.0):
            v0, ev0, te0, i0 = _sum(hip, gb, pbc, 0, cut)
            v1, ev1, te1, i1 = _sum(hip, gb, pbc, 1, cut)
            assert i0[:2] == [0, 0] and i0[3:] == [-1, -1, 0]                   # form 0 counts no slots
            assert i1[:2] == [1, 0] and i1[5] == 0
            assert i0[2] == i1[2] == (dev.N + 63) // 64
            assert np.array_equal(v0, v1), (name, pbc, cut, np.abs(v0 - v1).max())
            assert (ev0, te0) == (ev1, te1)
            assert te1 == dev.N * nq
            if cut == 0.0:
                assert ev1 == dev.N * nq - nq                                   # every pair but the self terms
            _dense(i1, ev1)
            assert i1[3] >= i1[4]
            scale = np.abs(w).max()
            assert np.abs(v1 - w).max() <= 1e-12 * scale
            if nq == 0:
                assert not v1.any() and i1[3] == i1[4] == 0
            if name == "random" and cut == 6.5:
                assert 0 < ev1 < dev.N * nq - nq
                print("2.5 nm, pbc %d: %d of %d pairs inside the cut-off; slots form 0 %d, form 1 %d (ratio %.3f)" % (pbc, ev1, te1, i1[3], i1[4], i1[3] / i1[4]))
    finally:
        _restore(L)


@pytest.mark.parametrize("pbc", [0, 1])
def test_cell_list_same_bits(cell_2p5, hip, pbc):
    """The cell-list kernel at its smallest shape (tile:4, 102.3 A laterally: 6 x 6 columns, reach 2), 4 % of the O sites charged.  Form 1 against form 0
    bit for bit with equal counters, two form-1 runs the same bits, against the all-pairs sum of the same call to 1e-15 of the largest potential and
    against the oracle to 1e-12 (test_pair_sum_cell_list's bounds)."""
    from devicekmc_amd import params as pm, structure
    host, L = hip
    k = 4
    s = structure.tile_structure(cell_2p5, k, 25.575, 25.575, 1440)
    p = pm.KMCParameters().for_tiling(k); p.pbc = bool(pbc)
    dev = host.Device(s, p, gpu_neighbors="cuda:0")
    gb = dev.make_gpubuf("cuda:0")
    assert dev.N == 150384
    rng = np.random.default_rng(17 + pbc)
    ok = dev.site_element == pm.O_EL
    q = np.where(ok & (rng.random(dev.N) < 0.04), rng.choice([-2, 2], dev.N), 0).astype(np.int32)
    put(gb, "site_charge", q)
    nq = int((q != 0).sum())
    assert nq >= 512                                                        # PW_MIN_CHARGED: below it the device takes k_pairwise
    want = _oracle_sum(dev.N, dev.site_x, dev.site_y, dev.site_z, p.lattice, pbc, p, q)
    try:
        vall, evall, teall, iall = _sum(hip, gb, pbc, 0, 0.0)
        v0, ev0, te0, i0 = _sum(hip, gb, pbc, 0, 6.5)
        v1, ev1, te1, i1 = _sum(hip, gb, pbc, 1, 6.5)
        v2, ev2, te2, i2 = _sum(hip, gb, pbc, 1, 6.5)
    finally:
        _restore(L)
    assert iall[:2] == [0, 0] and teall == dev.N * nq and evall == dev.N * nq - nq
    assert i0[:2] == [0, 1] and i0[3:] == [-1, -1, 0]
    assert i1[:2] == [1, 1] and i1[2] == i0[2] and 0 < i1[2] <= (dev.N + 63) // 64 + 36
    assert te1 < dev.N * nq                                                 # the cell list was taken
    assert np.array_equal(v0, v1), np.abs(v0 - v1).max()
    assert (ev0, te0) == (ev1, te1)
    assert np.array_equal(v1, v2) and (ev1, te1, i1) == (ev2, te2, i2)
    scale = np.abs(want).max()
    assert np.abs(vall - want).max() <= 1e-12 * scale
    assert np.abs(v1 - vall).max() <= 1e-15 * scale
    assert np.abs(v1 - want).max() <= 1e-12 * scale
    _dense(i1, ev1)
    assert i1[3] > i1[4]
    print("tile:4, pbc %d: %d charged, %d of %d tested pairs inside the cut-off; slots form 0 %d, form 1 %d (ratio %.3f)"
          % (pbc, nq, ev1, te1, i1[3], i1[4], i1[3] / i1[4]))


@pytest.fixture(scope="module")
def supersteps(hip):
    """Three coupled supersteps (current off) of 7.5nm and tile:4 under form 0 and under form 1, profiling on so that the kernel of every pair sum
    is on record."""
    import torch
    host, L = hip
    out = {}
    try:
        for name in ("7.5nm", "tile:4"):
            for form in (0, 1):
                L.dkmc_set_pair_form(form); L.dkmc_set_profiling(1)
                s, p, dev, sim, gb = _fresh(name)
                rec = []
                for k in range(3):
                    dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, k)
                    torch.cuda.synchronize()
                    st = host.get_stats()
                    step = dict(info=_info(L)[0], evaluated=st["pair_evaluated"], tested=st["pair_tested"], iters=st["cg_iters_K"],
                                pb=gb.site_potential_boundary.cpu().numpy().copy(), pc=gb.site_potential_charge.cpu().numpy().copy())
                    _, dt = sim.executeKMCStep(gb, dev, want_log=True)
                    step.update(log=np.array(sim.last_event_log).copy(), dt=dt, element=gb.site_element.cpu().numpy().copy(),
                                charge=gb.site_charge.cpu().numpy().copy())
                    rec.append(step)
                out[(name, form)] = rec
                del dev, sim, gb
                torch.cuda.empty_cache()
    finally:
        _restore(L)
    return out


@pytest.mark.parametrize("name", ["7.5nm", "tile:4"])
def test_coupled_supersteps_same_bits(supersteps, name):
    """Identical event logs, dt, elements, charges and both potentials; the counters too."""
    a, b = supersteps[(name, 0)], supersteps[(name, 1)]
    for k, (x, y) in enumerate(zip(a, b)):
        assert x["info"][0] == 0 and y["info"][0] == 1, k
        assert x["info"][1] == y["info"][1] and x["info"][2] == y["info"][2], k
        if name == "7.5nm":
            assert y["info"][1] == 0, k                                     # 2 x 2 columns: no cell list
        else:
            assert y["info"][1] == 1, k                                     # ~1 350 sites charged from the first step on
        assert (x["evaluated"], x["tested"]) == (y["evaluated"], y["tested"]), k
        assert x["iters"] == y["iters"], k
        assert np.array_equal(x["pb"], y["pb"]) and np.array_equal(x["pc"], y["pc"]), k
        assert len(x["log"]) > 0 and np.array_equal(x["log"], y["log"]), k
        assert x["dt"] == y["dt"], k
        assert np.array_equal(x["element"], y["element"]) and np.array_equal(x["charge"], y["charge"]), k
        print("%s step %d: kernel %d, %d charged, %d pairs evaluated" % (name, k, y["info"][1], int((y["charge"] != 0).sum()), y["evaluated"]))


def test_default_is_form_0(hip):
    host, L = hip
    try:
        assert L.dkmc_get_pair_form() == 0
        for v, want in ((1, 1), (2, 0), (-1, 0), (7, 0), (0, 0)):
            L.dkmc_set_pair_form(v)
            assert L.dkmc_get_pair_form() == want, v
    finally:
        _restore(L)
