"""The local heat model on the pattern-only CG of the K solve (dkmc_set_heat_form(1), csrc/heat.hip on csrc/kcg.hip's three forms) and its transient
sub-steps chained on the device.  Checked against the dense restatement of the model (oracle/heat_local.py, 2.5 nm), against the general CSR loop
(switch 0) and -- where no dense inverse fits -- by the TRUE scaled residual of the system built here from the neighbour index, the project's rule
for CG solutions.  The chain is checked bit for bit against the polled loop of the same switch.  The switches are read by constructLaplacian, so every
test sets them before building the device and resets them in a `finally`.  The model itself stays unpinned against the reference."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Vd = 5.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_1 = 50.0          # Device.h:117


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__ as g
    g.build()
    from devicekmc_amd import host, lib
    return host, lib.load()


def _reset(L):
    L.dkmc_set_heat_form(0); L.dkmc_debug_heat_chain(1, 0); L.dkmc_set_k_blocked(1); L.dkmc_set_k_blocked_large(0); L.dkmc_debug_kbw_segment_cap(0)


def _info(L):
    from devicekmc_amd import lib
    info = (C.c_longlong * 8)()
    lib.check(L.dkmc_get_heat_info(info))
    return dict(zip(("form", "rows", "words", "sub_steps", "syncs", "resumes", "bytes", "reserved"), list(info)))


@pytest.fixture(scope="module")
def ref_2p5(cell_2p5, hip):
    """The scenario of test_local_temperature_model, once: elements and (scaled) power of a real step of the 2.5 nm cell, and the dense oracle's
    temperatures after 3 transient sub-steps, 1 more from the heated state, and the steady state."""
    from devicekmc_amd import params as pm
    from oracle import heat_local as hl
    from test_gpu_parity import get, make_pair
    host, L = hip
    _reset(L)
    p = pm.KMCParameters(); p.solve_heating_local = True
    dev, sim, gb, o = make_pair(cell_2p5, p, hip, tol=1e-10)
    dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, 0)
    sim.executeKMCStep(gb, dev)
    dev.updatePower(gb, p, Vd)
    power = get(gb, "site_power").copy()
    element = get(gb, "site_element").copy()
    assert power.max() > 0
    orc = hl.LocalHeatOracle(element, dev.neigh_idx, p.metals, p.num_atoms_contact, p.nn_dist, p.delta, p.delta_t, p.tau, p.k_th_interface, p.k_th_metal)
    trial = np.full(dev.N, p.background_temp)
    orc.update_local_temperature(trial, power, element, p.background_temp, p.delta_t, p.tau, p.k_th_interface, p.k_th_vacancies, p.num_atoms_contact)
    power *= 30.0 / np.abs(trial - p.background_temp).max()
    T = np.full(dev.N, p.background_temp)
    stages = []
    for step_time in (2.5 * p.delta_t, 0.3 * p.delta_t, 2e3 * p.delta_t):
        Tbg, n, ss = orc.update_temperature_local(T, power, element, step_time, p.background_temp, p.delta_t, p.tau, p.k_th_interface,
                                                  p.k_th_vacancies, p.num_atoms_contact)
        stages.append(dict(step_time=step_time, T=T.copy(), Tbg=Tbg, n=n, steady=bool(ss)))
    assert np.abs(stages[1]["T"] - p.background_temp).max() > 1.0          # the comparison is not vacuous
    return dict(p=p, element=element, power=power, stages=stages, lo=orc.N_left_tot, hi=dev.N - orc.N_right_tot, m=orc.N_interface)


def _device_2p5(hip, cell, ref):
    """A fresh device of the 2.5 nm cell holding the scenario's elements and power, at the background temperature, Laplacian constructed."""
    from test_gpu_parity import put
    host, L = hip
    p = ref["p"]
    dev = host.Device(cell, p)
    gb = dev.make_gpubuf("cuda:0")
    dev.site_element = ref["element"]
    put(gb, "site_element", ref["element"]); put(gb, "site_power", ref["power"])
    put(gb, "site_temperature", np.full(dev.N, p.background_temp))
    dev.constructLaplacian(gb, p)
    assert dev.N_interface == ref["m"]
    return dev, gb


def _check_scenario(hip, cell, ref, want_form):
    """The three stages against the oracle, with the bounds of test_local_temperature_model (they follow from the 1e-10 stop tolerance of the solves)."""
    from test_gpu_parity import get
    host, L = hip
    p = ref["p"]
    dev, gb = _device_2p5(hip, cell, ref)
    for st in ref["stages"]:
        res = dev.updateTemperature(gb, p, st["step_time"])
        T = get(gb, "site_temperature")
        info = _info(L)
        assert (dev.last_heat_solves, dev.last_heat_steady) == (st["n"], st["steady"])
        assert info["form"] == want_form and info["rows"] == ref["m"] and info["sub_steps"] == st["n"] and info["reserved"] == 0, info
        assert dev.last_heat_info["form"] == want_form
        if not st["steady"]:
            err = np.abs(T - st["T"]).max()
            print("form %d  step_time %.3g: max |T - T_oracle| = %.3e K  iterations %d  syncs %d" % (want_form, st["step_time"], err, dev.last_heat_cg_iters, info["syncs"]))
            assert err <= 1e-7, err
            assert abs(res["Global temperature [K]"] - st["Tbg"]) <= 1e-9
            assert abs(float(gb.T_bg.item()) - st["Tbg"]) <= 1e-9
        else:
            rel = np.abs(T - st["T"]).max() / max(1.0, np.abs(st["T"] - p.background_temp).max())
            print("form %d  steady: relative error %.3e  iterations %d" % (want_form, rel, dev.last_heat_cg_iters))
            assert rel <= 1e-8, rel
            assert abs(res["Global temperature [K]"] - st["Tbg"]) <= 1e-8 * max(1.0, abs(st["Tbg"]))
        out = np.r_[0:ref["lo"], ref["hi"]:dev.N]
        assert np.all(T[out] == p.background_temp)
    return info


def test_blocked_form_against_the_dense_oracle(cell_2p5, hip, ref_2p5):
    """2.5 nm (9 399 sites, 3 000 interface rows): switch 1 runs on the blocked form (info: form 1), switch 0 on the general CSR loop (info: -1); both
    meet the oracle within the bounds of test_local_temperature_model."""
    host, L = hip
    try:
        _reset(L)
        L.dkmc_set_heat_form(1)
        assert L.dkmc_get_heat_form() == 1
        info = _check_scenario(hip, cell_2p5, ref_2p5, 1)
        assert info["words"] >= 32 * ref_2p5["m"] and info["bytes"] > 0
        L.dkmc_set_heat_form(0)
        info0 = _check_scenario(hip, cell_2p5, ref_2p5, -1)
        assert info0["resumes"] == 0
    finally:
        _reset(L)


def test_csr_positions_against_the_dense_oracle(cell_2p5, hip, ref_2p5):
    """The same with dkmc_set_k_blocked(0) at construct: the K-CG on the CSR positions of the heat pattern (info: form 0)."""
    host, L = hip
    try:
        _reset(L)
        L.dkmc_set_heat_form(1); L.dkmc_set_k_blocked(0)
        _check_scenario(hip, cell_2p5, ref_2p5, 0)
    finally:
        _reset(L)


@pytest.mark.parametrize("k_blocked", [1, 0])
def test_chain_equals_polled_bit_for_bit(cell_2p5, hip, ref_2p5, k_blocked):
    """41 transient sub-steps (step_time = 40.5 delta_t: three batches of at most 16).  A launch that is skipped changes no data, so the chained
    update gives the bits of the polled one, whatever the budget.  Synchronisations: one per chained batch plus one per resumed sub-step (the resumed
    solve enqueues what the largest solve so far needed before its first poll); a failure ends its batch early, so there are at most
    ceil(41 / 16) + resumes batches."""
    from test_gpu_parity import get, put
    host, L = hip
    p = ref_2p5["p"]
    n_sub = 41
    try:
        _reset(L)
        L.dkmc_set_heat_form(1); L.dkmc_set_k_blocked(k_blocked)
        dev, gb = _device_2p5(hip, cell_2p5, ref_2p5)

        def run(on, budget, step_time=40.5 * p.delta_t, reset=True):
            L.dkmc_debug_heat_chain(on, budget)
            if reset:
                put(gb, "site_temperature", np.full(dev.N, p.background_temp))
            dev.updateTemperature(gb, p, step_time)
            return get(gb, "site_temperature").copy(), dev.last_heat_cg_iters, _info(L)

        T_pol, it_pol, i_pol = run(0, 0)
        assert dev.last_heat_solves == n_sub and i_pol["sub_steps"] == n_sub and i_pol["resumes"] == 0 and i_pol["form"] == (1 if k_blocked else 0)
        assert i_pol["syncs"] >= n_sub
        assert np.abs(T_pol - p.background_temp).max() > 1.0
        # the polled counts, sub-step by sub-step (41 updates of one sub-step each: the same solves), all above the forced budget of 8
        put(gb, "site_temperature", np.full(dev.N, p.background_temp))
        counts = [run(0, 0, 0.5 * p.delta_t, reset=False)[1] for _ in range(n_sub)]
        assert np.array_equal(get(gb, "site_temperature"), T_pol) and sum(counts) == it_pol
        assert min(counts) > 8, counts
        # default budget
        T_a, it_a, i_a = run(1, 0)
        T_b, it_b, i_b = run(1, 0)
        print("polled: %d iterations, %d syncs; chained: %d syncs, %d resumes; counts %d..%d" % (it_pol, i_pol["syncs"], i_a["syncs"], i_a["resumes"], min(counts), max(counts)))
        assert np.array_equal(T_a, T_pol) and it_a == it_pol
        assert np.array_equal(T_b, T_a) and it_b == it_a and i_b == i_a
        assert i_a["syncs"] <= 3 + i_a["resumes"], i_a
        # a budget below what any solve needs: every sub-step takes the resume path
        T_c, it_c, i_c = run(1, 8)
        assert np.array_equal(T_c, T_pol) and it_c == it_pol
        assert i_c["resumes"] > 0
        batches = 3 + i_c["resumes"]
        assert i_c["syncs"] <= n_sub + batches, i_c
    finally:
        _reset(L)


# ---- systems without a dense oracle: the TRUE scaled residual ----------------------------------------------------------------------------------
def _heat_matrix(neigh, element, metals, lo, m, gamma):
    """L of the local model (the comment at the head of the local model in csrc/heat.hip): 1 per neighbour pair inside the interface [lo, lo + m),
    diagonal -gamma [a neighbour, inside or not, is metallic] - degree."""
    import scipy.sparse as sp
    rows = np.asarray(neigh[lo:lo + m])
    valid = rows >= 0
    inside = valid & (rows >= lo) & (rows < lo + m)
    deg = inside.sum(axis=1)
    ism = np.isin(element, list(metals))
    bnd = (valid & ism[np.where(valid, rows, 0)]).any(axis=1)
    diagL = -gamma * bnd - deg
    ri = np.repeat(np.arange(m), deg)
    adj = sp.csr_matrix((np.ones(len(ri)), (ri, rows[inside] - lo)), shape=(m, m))
    return (adj + sp.diags(diagL)).tocsr()


def _scaled_residual(A, y, b):
    return float(np.linalg.norm((A @ y - b) / np.sqrt(A.diagonal())))


def _smooth_power(dev, p, lo, m, c):
    """A smooth positive field on the interface whose one transient sub-step heats by at most 30 K (|(I - s L)^-1|_inf <= 1)."""
    x, y, z = (np.asarray(a, dtype=np.float64) for a in (dev.site_x, dev.site_y, dev.site_z))
    f = (1.5 + np.cos(2 * np.pi * y / (np.ptp(y) + 1.0)) * np.cos(2 * np.pi * z / (np.ptp(z) + 1.0))) * np.exp(-((x - x.mean()) / (0.25 * np.ptp(x) + 1.0)) ** 2)
    P = np.zeros(dev.N)
    P[lo:lo + m] = f[lo:lo + m]
    P *= 30.0 / (np.abs(P[lo:lo + m] * c).max() * p.delta_t * p.tau * abs(T_1 - p.background_temp))
    return P


def _build(hip, name):
    sys.path.insert(0, ROOT)
    from bench import make_workload
    host, L = hip
    s, p = make_workload(name)
    p.solve_current = False; p.solve_heating_global = False; p.solve_heating_local = True
    dev = host.Device(s, p, gpu_neighbors="cuda:0")
    gb = dev.make_gpubuf("cuda:0")
    return p, dev, gb


def _system(dev, p):
    from devicekmc_amd.params import VACANCY
    lo, m = dev.N_left_tot, dev.N_interface
    gamma = 1.0 / (p.delta * ((p.k_th_interface / p.k_th_metal) + 1.0))
    Lm = _heat_matrix(dev.neigh_idx, dev.site_element, p.metals, lo, m, gamma)
    pv = 1.0 / ((p.nn_dist * 1e-10 * p.k_th_interface) * (T_1 - p.background_temp))
    pn = 1.0 / ((p.nn_dist * 1e-10 * p.k_th_vacancies) * (T_1 - p.background_temp))
    c = np.where(np.asarray(dev.site_element)[lo:lo + m] == VACANCY, pv, pn)
    return lo, m, Lm, c


def _transient_residual(dev, gb, p, Lm, c, lo, m, P, T_before):
    """One transient sub-step from T_before; the scaled residual of (I - s L) y = T_vec + P c s with y recovered from the new temperatures."""
    import scipy.sparse as sp
    from test_gpu_parity import get, put
    T0, s = p.background_temp, p.delta_t * p.tau
    put(gb, "site_temperature", T_before)
    dev.updateTemperature(gb, p, 0.5 * p.delta_t)
    assert dev.last_heat_solves == 1 and not dev.last_heat_steady
    T = get(gb, "site_temperature").copy()
    A = (sp.identity(m) - s * Lm).tocsr()
    b = (T_before[lo:lo + m] - T0) / (T_1 - T0) + P[lo:lo + m] * c * s
    return T, _scaled_residual(A, (T[lo:lo + m] - T0) / (T_1 - T0), b)


def test_7p5_blocked_form_true_residual(hip):
    """7.5 nm (85 071 sites, 27 000 interface rows), blocked form: one transient sub-step and the steady solve meet the stop test in the true scaled
    residual, ||D^-1/2 (A y - b)|| <= 10 tol (tol = 1e-10, the factor of the K tests); switch 0 and 1 agree to 1e-7 K on the transient sub-step."""
    from test_gpu_parity import get, put
    host, L = hip
    tol = 1e-10
    out = {}
    try:
        for form in (1, 0):
            _reset(L)
            L.dkmc_set_heat_form(form)
            p, dev, gb = _build(hip, "7.5nm")
            dev.constructLaplacian(gb, p)
            lo, m, Lm, c = _system(dev, p)
            assert dev.N == 85071 and m == 27000
            P = _smooth_power(dev, p, lo, m, c)
            put(gb, "site_power", P)
            T0 = p.background_temp
            T, res = _transient_residual(dev, gb, p, Lm, c, lo, m, P, np.full(dev.N, T0))
            info = _info(L)
            print("7.5nm switch %d: transient scaled residual %.3e  iterations %d  max rise %.3f K" % (form, res, dev.last_heat_cg_iters, np.abs(T - T0).max()))
            assert info["form"] == (1 if form else -1) and info["rows"] == m
            assert res <= 10 * tol, res
            assert np.abs(T - T0).max() > 1.0
            out[form] = T
            if form:
                # steady: the power scaled (the model is linear in it) so that the rise stays at 30 K and y is recovered from T to 1e-16
                put(gb, "site_temperature", np.full(dev.N, T0))
                dev.updateTemperature(gb, p, 2e3 * p.delta_t)
                rise = np.abs(get(gb, "site_temperature") - T0).max()
                assert dev.last_heat_steady and rise > 0
                P2 = P * (30.0 / rise)
                put(gb, "site_power", P2); put(gb, "site_temperature", np.full(dev.N, T0))
                dev.updateTemperature(gb, p, 2e3 * p.delta_t)
                Ts = get(gb, "site_temperature")
                res_s = _scaled_residual((-Lm).tocsr(), (Ts[lo:lo + m] - T0) / (T_1 - T0), P2[lo:lo + m] * c)
                print("7.5nm steady: scaled residual %.3e  iterations %d  rise %.3f K" % (res_s, dev.last_heat_cg_iters, np.abs(Ts - T0).max()))
                assert _info(L)["form"] == 1 and _info(L)["sub_steps"] == 1
                assert res_s <= 10 * tol, res_s
            del dev, gb
        d = np.abs(out[1] - out[0]).max()
        print("7.5nm: max |T(switch 1) - T(switch 0)| = %.3e K" % d)
        assert d <= 1e-7, d
    finally:
        _reset(L)


def test_windowed_form_and_refused_build(hip):
    """tile:10 (939 900 sites, 300 000 interface rows: the smallest tiling whose interface exceeds 262 144 rows -- it grows as 3 000 k^2) with
    dkmc_set_k_blocked_large(1): the windowed blocked form (info: form 2); reconstructed with the segment cap forced to 1 the builder refuses and the
    solves run on the CSR positions (form 0).  One transient sub-step each, checked by the true scaled residual.  Current off: synthetic power."""
    from test_gpu_parity import put
    host, L = hip
    tol = 1e-10
    try:
        _reset(L)
        L.dkmc_set_heat_form(1); L.dkmc_set_k_blocked_large(1)
        p, dev, gb = _build(hip, "tile:10")
        dev.constructLaplacian(gb, p)
        lo, m, Lm, c = _system(dev, p)
        assert m > 262144
        P = _smooth_power(dev, p, lo, m, c)
        put(gb, "site_power", P)
        T0 = p.background_temp
        for cap, want in ((0, 2), (1, 0)):
            if cap:
                L.dkmc_debug_kbw_segment_cap(cap)
                dev.constructLaplacian(gb, p)
            T, res = _transient_residual(dev, gb, p, Lm, c, lo, m, P, np.full(dev.N, T0))
            info = _info(L)
            print("tile:10 form %d: transient scaled residual %.3e  iterations %d  words %d" % (info["form"], res, dev.last_heat_cg_iters, info["words"]))
            assert info["form"] == want and info["rows"] == m, info
            assert res <= 10 * tol, res
            assert np.abs(T - T0).max() > 1.0
    finally:
        _reset(L)
