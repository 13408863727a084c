"""What update_power and the global temperature update make of a solved current system, against the host evaluation of the definitions
(power_ref.py: the reference and the derived bounds; validated without a GPU by test_power_ref.py): the dissipated power per site in both forms of
X (k_power<64>; k_xt_gather_S + the rectified tile pass + k_xt_rows<1> + k_xt_power_rows), I_macro (k_imacro), the shift of the node potentials
(k_min_m, k_shift) and both closed forms of the global temperature (k_power_partials, k_temp_update).  Everything is a deterministic function of data
read back after the call -- the exported X, atom_virtual_potentials, site_power -- so every comparison is per site, at a few hundred ulps, and does
not depend on how far the CG got.  Every case prints its worst |gpu - ref| / bound."""
import ctypes as C
import math

import numpy as np
import pytest

import current_map_ref as cmr
import power_ref as pr
from conftest import params_7p5

pytestmark = pytest.mark.gpu

SENTINEL = -7.0


@pytest.fixture(scope="module")
def hip():
    import torch
    import __graft_entry__ as g
    g.build()
    from devicekmc_amd import host, lib
    assert torch.cuda.is_available()
    return host, lib.load()


def get(gb, name):
    return gb.t[name].cpu().numpy()


def put(gb, name, arr):
    import torch
    t = gb.t[name]
    t.copy_(torch.as_tensor(np.ascontiguousarray(arr)).to(t.dtype))


def _run(hip, structure, p, V, fmt=1, heating=True, vacancies=0, start=None, keep=False):
    """fresh device -> (extra vacancies from default_rng(5)) -> Laplace -> charge -> potential -> site_power filled with the sentinel -> update_power.
    start: the single-vector loop at a tolerance it meets at once, from this vector (warm-start mode 0 reads the buffer).  Returns everything the
    checks read back."""
    from devicekmc_amd import params as pm
    host, L = hip
    p.solve_heating_global = heating
    dev = host.Device(structure, p); gb = dev.make_gpubuf("cuda:0")
    if vacancies:
        el = dev.site_element.copy()
        el[np.random.default_rng(5).choice(np.nonzero(el == pm.O_EL)[0], vacancies, replace=False)] = pm.VACANCY
        dev.site_element = el
    dev.setLaplacePotential(gb, p, V); gb.sync_HostToGPU(dev)
    dev.updateCharge(gb); dev.updatePotential(gb, p, V, 0)
    put(gb, "site_power", np.full(dev.N, SENTINEL))
    tol = p.cg_tol
    try:
        L.dkmc_set_x_format(fmt)
        if start is not None:
            L.dkmc_set_current_warm_start(0); L.dkmc_set_x_block(1)
            p.cg_tol = 1e30
            put(gb, "atom_virtual_potentials", start)
        dev.updatePower(gb, p, V)
    finally:
        L.dkmc_set_x_format(1); L.dkmc_set_current_warm_start(1); L.dkmc_set_x_block(16); L.dkmc_set_cg_tolerance(1e-6)
        p.cg_tol = tol
    el = get(gb, "site_element")
    site = cmr.atom_sites(el)
    rec = dict(V=V, fmt=fmt, heating=heating, N=dev.N, Na=dev.N_atom, imacro=dev.imacro, X=host.get_last_X(), m=get(gb, "atom_virtual_potentials").copy(),
               power=get(gb, "site_power").copy(), site=site, metal=np.isin(el[site], p.metals), xt_ns=host.get_stats()["xt_ns"],
               iters=host.get_stats()["cg_iters_X"], pos=(get(gb, "atom_x"), get(gb, "atom_y"), get(gb, "atom_z")), p=p)
    assert len(site) == rec["Na"] and len(rec["X"][0]) - 1 == rec["Na"] + 1 and len(rec["m"]) == rec["Na"] + 2
    if keep:
        rec["dev"], rec["gb"] = dev, gb
    return rec


def _ratio(diff, bound):
    """worst |diff| / bound; where the bound is zero the values must agree exactly"""
    diff, bound = np.atleast_1d(diff), np.atleast_1d(bound)
    assert np.all(diff[bound == 0] == 0)
    return float((diff[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def _check_power(rec, label):
    """The assertions every heating-on run makes: each written site within its bound of the reference evaluated on the exported X and the potentials
    read back, every other site still the sentinel bit for bit, every written value >= 0.  Returns (ref, written, bound, entries)."""
    assert rec["heating"]
    e = pr.heating_entries(rec["X"], rec["m"], rec["V"])
    ref, written, bound = pr.site_power_reference(rec["X"], rec["m"], rec["V"], rec["site"], rec["metal"], rec["N"], entries=e)
    pw = rec["power"]
    assert written.sum() == (~rec["metal"][:rec["Na"] - 1]).sum() > 0
    assert np.array_equal(pw[~written].view(np.int64), np.full((~written).sum(), SENTINEL).view(np.int64))
    assert np.all(pw[written] >= 0) and ref.max() > 0
    ratio = _ratio(np.abs(pw - ref)[written], bound[written])
    low = written & (ref < 1e-6 * ref.max())
    print("%s: site power, worst |gpu - ref| / bound = %.3g over %d written sites (%d below 1e-6 of the largest, smallest %.3g of it)"
          % (label, ratio, written.sum(), low.sum(), ref[written].min() / ref.max()))
    assert ratio <= 1, label
    return ref, written, bound, e


def _check_imacro(rec, label):
    val, bound, terms = pr.imacro_reference(rec["X"], rec["m"])
    assert not rec["heating"] and len(terms) > 0
    ratio = _ratio(abs(rec["imacro"] - val), bound)
    print("%s: I_macro, |gpu - ref| / bound = %.3g (%d terms)" % (label, ratio, len(terms)))
    assert ratio <= 1, label


def _check_pair(off, on, label):
    """heating off against heating on, same state: I_macro the same bits (step 6 precedes the shift, the solve is bit-reproducible), the potentials of
    the heating-on run the shifted ones of the other, bit for bit; and a heating-off run writes no power at all"""
    assert not off["heating"] and on["heating"] and off["iters"] == on["iters"]
    assert np.float64(off["imacro"]).tobytes() == np.float64(on["imacro"]).tobytes(), label
    Na = off["Na"]
    want = pr.shift_reference(off["m"], Na)
    assert on["m"][:Na + 2].tobytes() == want.tobytes(), label
    assert np.array_equal(off["power"].view(np.int64), np.full(off["N"], SENTINEL).view(np.int64))
    print("%s: shift by %.6g, the smallest of %d potentials: the same bits" % (label, abs(off["m"][2:Na + 2].min()), Na))


class _Runs:
    """the solves of the 2.5 nm cell with 300 extra vacancies (cg_tol 1e-10, default block width), each run once and shared by the tests"""

    def __init__(self, hip, cell):
        self.hip, self.cell, self.done = hip, cell, {}

    def __call__(self, fmt, V, heating, rough=False):
        from devicekmc_amd import params as pm
        key = (fmt, V, heating, rough)
        if key not in self.done:
            p = pm.KMCParameters(); p.cg_tol = 1e-10
            start = self.rough_start(fmt, V) if rough else None
            self.done[key] = _run(self.hip, self.cell, p, V, fmt=fmt, heating=heating, vacancies=300, start=start, keep=(key == (1, 5.0, True, False)))
        return self.done[key]

    def tunnelling(self, rec, r, c):
        p = rec["p"]
        return cmr.site_dist(*rec["pos"], r - 2, c - 2, p.lattice[1], p.lattice[2], int(p.pbc)) >= p.nn_dist

    def rough_start(self, fmt, V):
        """a start vector that is nothing like a solution: default_rng(17), magnitudes log-uniform in [1e-12, 1e-8] with random signs, and 64
        planted equal pairs on distinct nodes, half of them neighbour pairs and half pairs of the tunnelling set (the pattern is that of the regular
        solve of the same state)"""
        rec = self(fmt, V, False)
        rng = np.random.default_rng(17)
        n = rec["Na"] + 2
        v = 10.0 ** rng.uniform(-12, -8, n) * rng.choice([-1.0, 1.0], n)
        rp, ci, _ = rec["X"]
        rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
        ci = ci.astype(np.int64)
        up = (rows >= 2) & (ci > rows)
        r, c = rows[up], ci[up]
        tun = self.tunnelling(rec, r, c)
        used = set()
        for kind in (~tun, tun):
            k = np.flatnonzero(kind)
            planted = 0
            for j in rng.permutation(k):
                a, b = int(r[j]), int(c[j])
                if a in used or b in used:
                    continue
                used.update((a, b)); v[b] = v[a]; planted += 1
                if planted == 32:
                    break
            assert planted == 32
        return v


@pytest.fixture(scope="module")
def runs(hip, cell_2p5):
    return _Runs(hip, cell_2p5)


FMT = {"tiled": 1, "csr": 0}


@pytest.mark.parametrize("V", [5.0, -3.0])
@pytest.mark.parametrize("fmt", ["tiled", "csr"])
def test_site_power_2p5(runs, hip, fmt, V):
    """(a) 2.5 nm cell + 300 vacancies, both forms of X, both signs of the bias.  The existing comparison with the oracle, 1e-6 of the largest value,
    says nothing about most of these sites: more than 2000 of the 3000 written ones lie below that line; and at least 300 rows -- the vacancy rows,
    which receive tile sums in the tiled form -- have more than 100 heating terms."""
    rec = runs(FMT[fmt], V, True)
    ref, written, bound, e = _check_power(rec, "2.5 nm %s %+g V" % (fmt, V))
    assert rec["xt_ns"] > 0
    assert (written & (ref < 1e-6 * ref.max())).sum() > 2000
    _, _, num = pr.row_sums(e)
    wr = np.zeros(e["n"], dtype=bool); wr[2:][~rec["metal"][:rec["Na"] - 1]] = True
    assert (num[wr] > 100).sum() >= 300


@pytest.mark.parametrize("case", ["few_vacancies", "no_vacancies", "empty_S", "small_bias"])
def test_site_power_degenerate_tunnelling_sets(cell_2p5, hip, case):
    """(b) the recipes of test_tiled_X_edge_cases on the tiled form: very few vacancies, none (S = contact metals only), an empty S (no tile launch at
    all: the row kernel alone) and a bias so small that only ragged cells are left."""
    from devicekmc_amd import params as pm
    p = pm.KMCParameters(); p.cg_tol = 1e-10
    if case == "few_vacancies":
        p.initial_vacancy_concentration = 0.002
    if case in ("no_vacancies", "empty_S"):
        p.initial_vacancy_concentration = 0.0
    if case == "empty_S":
        p.num_layers_contact = 100
    rec = _run(hip, cell_2p5, p, 0.03 if case == "small_bias" else 5.0)
    assert (rec["xt_ns"] == 0) == (case == "empty_S")
    _check_power(rec, case)


@pytest.fixture(scope="module")
def pair_7p5(hip, dev_7p5):
    return {h: _run(hip, dev_7p5, params_7p5(), 5.0, heating=h) for h in (False, True)}


def test_site_power_and_shift_7p5(pair_7p5):
    """(c), (f) 85 071 sites, tiled: the smallest fixture with multi-strip runs, records shared by four waves, a padded S and partial tiles; Na + 2 is
    above 32 768, where k_min_m takes its stride."""
    off, on = pair_7p5[False], pair_7p5[True]
    assert on["N"] == 85071 and on["Na"] + 2 > 32768 and on["xt_ns"] > 0
    ref, written, bound, e = _check_power(on, "7.5 nm tiled +5 V")
    assert (written & (ref < 1e-6 * ref.max())).sum() > 2000
    _, _, num = pr.row_sums(e)
    wr = np.zeros(e["n"], dtype=bool); wr[2:][~on["metal"][:on["Na"] - 1]] = True
    assert (num[wr] > 100).sum() >= 300
    _check_imacro(off, "7.5 nm tiled +5 V")
    _check_pair(off, on, "7.5 nm tiled +5 V")


@pytest.mark.parametrize("V", [5.0, -3.0])
@pytest.mark.parametrize("fmt", ["tiled", "csr"])
def test_imacro_and_shift_2p5(runs, fmt, V):
    """(e), (f) the heating-off run leaves in the buffer exactly what k_imacro read: I_macro within its bound of the rule evaluated there; the
    heating-on run of the same state has the same I_macro bits and the shifted potentials bit for bit."""
    off, on = runs(FMT[fmt], V, False), runs(FMT[fmt], V, True)
    label = "2.5 nm %s %+g V" % (fmt, V)
    _check_imacro(off, label)
    assert (off["imacro"] > 0) == (V > 0)
    _check_pair(off, on, label)


@pytest.mark.parametrize("V", [5.0, -3.0])
@pytest.mark.parametrize("fmt", ["tiled", "csr"])
def test_rough_potentials(runs, fmt, V):
    """(d) A solved m is smooth: neighbouring potentials differ little and every pair of S heats the same end.  Both branches of the rectifier, the
    sign handling and near-ties inside tiles need a vector that is not: the single-vector loop is started from a random vector with planted equal
    pairs at a tolerance it meets at or near its start, and whatever it leaves in the buffer is what the reference evaluates."""
    off, on = runs(FMT[fmt], V, False, rough=True), runs(FMT[fmt], V, True, rough=True)
    label = "rough %s %+g V" % (fmt, V)
    ref, written, bound, e = _check_power(on, label)
    # still rough: of the pairs of S that heat an end (stored once above the diagonal), more than 40 % heat the column end, more than 40 % the row end
    up = e["c"] > e["r"]
    tun = np.zeros(len(up), dtype=bool)
    tun[up] = runs.tunnelling(on, e["r"][up], e["c"][up])
    sel = tun & (e["ical"] != 0)
    assert sel.sum() > 10000
    row_end = e["heat"][sel].mean()
    ties = int((tun & (e["ical"] == 0) & (e["x"] != 0)).sum())
    print("%s: %d sweeps, %d heating pairs of S, %.1f %% heat their row end; %d pairs of S at equal potentials" % (label, on["iters"], sel.sum(), 100 * row_end, ties))
    assert 0.4 < row_end < 0.6
    _check_imacro(off, label)
    _check_pair(off, on, label)
    m = off["m"][2:off["Na"] + 2]
    assert -m.min() > 0.1 * np.abs(m).max()                             # the minimum is strongly negative


def _temperature_constants():
    from devicekmc_amd import params as pm
    p = pm.KMCParameters()
    Cth = p.A * p.t_ox * p.c_p * 1e6
    a = -p.dissipation_constant / Cth * p.small_step + 1; b = p.dissipation_constant / Cth * p.small_step * p.background_temp
    return p, Cth, a, b


def _temperature_calls(hip, power, check_P, label, modes=(0, 1)):
    """both entry points on a float64 device tensor, over the steps and start temperatures of the issue.  check_P(P) asserts on the P_tot returned
    and gives the P the reference is evaluated at.  Returns the worst |T - ref| / bound per mode and the largest rise in units of its bound."""
    import torch
    host, L = hip
    from devicekmc_amd.lib import check
    p, Cth, a, b = _temperature_constants()
    dev = torch.device("cuda:0")
    host._use_stream(dev)
    d_p = torch.as_tensor(power, dtype=torch.float64).to(dev)
    d_T = torch.zeros(1, dtype=torch.float64, device=dev)
    N = len(power)
    worst, rise = {0: 0.0, 1: 0.0}, 0.0
    P_ref = None
    for T0 in (300.0, 812.5):
        for t in (1e-13, 1e-9, 1e-7, 1e-3):
            d_T.fill_(T0)
            P = C.c_double(-1.0)
            check(L.dkmc_update_temperature_global_analytic(host._ptr(d_p), host._ptr(d_T), N, t, p.dissipation_constant, p.t_ox, p.A, p.c_p, C.byref(P)))
            P_ref = check_P(P.value)
            T, bound, _ = pr.temperature_reference(0, P_ref, T0, event_time=t, dissipation_constant=p.dissipation_constant, C=Cth)
            got = float(d_T.item())
            assert abs(got - T) <= bound, (label, 0, T0, t, got, T, bound)
            worst[0] = max(worst[0], abs(got - T) / bound); rise = max(rise, abs(T - T0) / bound)
        for s in (0, 1, 10000.5, 1e9) if 1 in modes else ():
            d_T.fill_(T0)
            check(L.dkmc_update_temperatureglobal_gpu(host._ptr(d_p), host._ptr(d_T), N, a, b, s, Cth, p.small_step))
            T, bound, _ = pr.temperature_reference(1, P_ref, T0, a_coeff=a, b_coeff=b, number_steps=s, C_thermal=Cth, small_step=p.small_step)
            got = float(d_T.item())
            assert abs(got - T) <= bound, (label, 1, T0, s, got, T, bound)
            worst[1] = max(worst[1], abs(got - T) / bound); rise = max(rise, abs(T - T0) / bound)
    return worst, rise


@pytest.mark.parametrize("N", [1, 63, 64, 255, 256, 257, 1023, 262144, 262145, 262144 + 785, 600001])
def test_global_temperature_on_synthetic_power(hip, N):
    """(g) k_power_partials and k_temp_update called directly: one workgroup, a partial one, the cap of 1024 workgroups at 262 144 sites and the
    grid-stride path beyond it; steps long enough for the exponential / the power to matter.
    Array 1 is exactly summable: integers below 2^20 times 2^-90, the last two raised by 2^52 and 2^51 (N = 1: the one by 2^52) so that the sum, about
    5.5e-12 W, is of the size of a real one and still below 2^53 units: every partial sum in any order is exact, so P_tot is the exact sum bit for
    bit and T_bg of both modes is within its bound of the reference at that P.
    Array 2 is realistic: log-uniform over 13 decades, sum near 1e-11 W: P_tot within the summation bound of fsum, T_bg (mode 0) within its bound of the
    reference at the returned P_tot."""
    rng = np.random.default_rng(N)
    k = [int(v) for v in rng.integers(0, 2 ** 20, N)]
    k[-1] += 2 ** 52
    if N > 1:
        k[-2] += 2 ** 51
    total = sum(k)
    assert total < 2 ** 53
    exact = math.ldexp(float(total), -90)
    p1 = np.array([math.ldexp(float(v), -90) for v in k])

    def same_bits(P):
        assert np.float64(P).tobytes() == np.float64(exact).tobytes(), (N, P, exact)
        return exact

    worst, rise = _temperature_calls(hip, p1, same_bits, "exact N=%d" % N)
    print("N = %d, exactly summable: P_tot the same bits; T_bg worst |gpu - ref| / bound: mode 0 %.3g, mode 1 %.3g; largest rise %.3g bounds" % (N, worst[0], worst[1], rise))
    assert rise > 1e12

    p2 = 10.0 ** rng.uniform(-13, 0, N)
    p2 *= 1e-11 / math.fsum(p2)
    want, sb = math.fsum(p2), pr.power_sum_bound(p2)
    seen = []

    def within(P):
        assert abs(P - want) <= sb, (N, P, want, sb)
        seen.append(abs(P - want) / sb)
        return P

    worst, rise = _temperature_calls(hip, p2, within, "realistic N=%d" % N, modes=(0,))
    print("N = %d, 13 decades: |P_tot - fsum| / bound = %.3g; T_bg (mode 0) worst |gpu - ref| / bound %.3g" % (N, max(seen), worst[0]))
    # not vacuous: 1e-11 W for 1e-7 s is a rise of about 14 K against a bound of about 1.2e-12 K
    pp, Cth, _, _ = _temperature_constants()
    T, bound, _ = pr.temperature_reference(0, want, 300.0, event_time=1e-7, dissipation_constant=pp.dissipation_constant, C=Cth)
    assert 13.0 < T - 300.0 < 15.0 and bound < 1.3e-12 and rise > 1e13


def test_global_temperature_on_real_power(runs, hip):
    """(h) after (a), tiled, +5 V: updateTemperature with a step of 1e-6 s.  The total power it reports is the sum of site_power within the summation
    bound, and T_bg is within the formula bound of the reference at that power."""
    host, L = hip
    from devicekmc_amd.lib import check
    rec = runs(1, 5.0, True)
    dev, gb, p = rec["dev"], rec["gb"], rec["p"]
    pw = np.where(rec["power"] == SENTINEL, 0.0, rec["power"])         # (the sites no kernel writes are zero in a run that did not plant the sentinel)
    assert np.all(pw >= 0)
    put(gb, "site_power", pw)
    T0 = float(gb.T_bg.item())
    assert T0 == p.background_temp
    out = dev.updateTemperature(gb, p, 1e-6)
    # the same call again from the same T_bg, for the unrounded P_tot (updateTemperature reports it in mW)
    gb.copy_Tbg_toGPU(T0)
    P = C.c_double(-1.0)
    check(L.dkmc_update_temperature_global_analytic(host._ptr(gb.site_power), host._ptr(gb.T_bg), gb.N_, 1e-6, p.dissipation_constant, p.t_ox, p.A, p.c_p,
                                                    C.byref(P)))
    assert float(gb.T_bg.item()) == dev.T_bg == out["Global temperature [K]"] and out["Total dissipated power [mW]"] == P.value * 1e3
    want, sb = math.fsum(pw), pr.power_sum_bound(pw)
    assert abs(P.value - want) <= sb
    T, bound, _ = pr.temperature_reference(0, P.value, T0, event_time=1e-6, dissipation_constant=p.dissipation_constant, C=p.A * p.t_ox * p.c_p * 1e6)
    print("real power: P_tot = %.6g W, |P_tot - fsum| / bound = %.3g; T_bg rise %.6g K, |gpu - ref| / bound = %.3g"
          % (P.value, abs(P.value - want) / sb, T - T0, abs(dev.T_bg - T) / bound))
    assert abs(dev.T_bg - T) <= bound and T - T0 > 1e6 * bound
