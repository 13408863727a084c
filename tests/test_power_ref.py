"""The host reference of the dissipated power, I_macro, the shift and the global temperature (tests/power_ref.py), validated without a GPU on the
CPU oracle's X and potentials of the 2.5 nm cell with 300 extra vacancies at +5 V and -3 V: it is the oracle's definition, its bounds hold for any
summation order, it resolves the entries it sums (four seeded faults leave the bound on sites far below the largest power), and plain fp64
evaluations of the two closed forms stay within the stated bound of the 60-digit value."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import current_map_ref as cmr
import power_ref as pr

U = pr.U
SENTINEL = -7.0


@pytest.fixture(scope="module", params=[5.0, -3.0], ids=["+5V", "-3V"])
def case(request, cell_2p5):
    """oracle state -> X, the unshifted and the shifted potentials, the oracle's power (on a sentinel) and I_macro"""
    from devicekmc_amd import params as pm
    from oracle import oracle as oc
    V = request.param
    p = pm.KMCParameters(); p.cg_tol = 1e-10; p.solve_heating_global = True
    o = oc.OracleKMC(cell_2p5.element, cell_2p5.x, cell_2p5.y, cell_2p5.z, p)
    el = o.element.copy()
    el[np.random.default_rng(5).choice(np.nonzero(el == pm.O_EL)[0], 300, replace=False)] = pm.VACANCY
    o.element[:] = el
    o.set_laplace_potential(V); o.update_charge(); o.update_potential(V)
    imacro = o.update_power(V, heating=False)
    Xo = o.last_X; Na = Xo["Na"]
    m0 = o.virtual_potentials[:Na + 2].copy()
    m = m0.copy()
    power = np.full(o.N, SENTINEL)
    oc.lib().okmc_dissipated_power(Na, oc._p(Xo["row_ptr"]), oc._p(Xo["col"]), oc._p(Xo["data"]), oc._p(m), C.c_double(V), oc._p(Xo["ael"]),
                                   oc._p(Xo["atom_site"]), oc._p(o.metals), len(o.metals), C.c_double(1.0), oc._p(power))
    X = (Xo["row_ptr"], Xo["col"], Xo["data"])
    metal = np.isin(Xo["ael"], p.metals)
    site = Xo["atom_site"]
    e = pr.heating_entries(X, m, V)
    ref = pr.site_power_reference(X, m, V, site, metal, o.N, entries=e)
    return dict(V=V, p=p, N=o.N, Na=Na, X=X, m0=m0, m=m, power=power, imacro=imacro, metal=metal, site=site, ael=Xo["ael"], e=e, ref=ref,
                ax=o.x[site], ay=o.y[site], az=o.z[site])


def test_reference_is_the_oracles_definition(case):
    """against okmc_dissipated_power within the oracle's own bound: it sums v m_c and (sum v) m_i, which cancel, 4 n_i u sum |v| (|m_c| + |m_i|)"""
    ref, written, bound = case["ref"]
    e, m, o = case["e"], case["m"], case["power"]
    assert np.array_equal(m, pr.shift_reference(case["m0"], case["Na"]))              # the shift: one addition per element, the same bits
    assert np.array_equal(written, o != SENTINEL) and written.sum() == 3000
    assert np.all(ref[written] >= 0) and ref.max() > 0
    h = e["heat"]
    w = np.abs(e["ical"][h]) * (np.abs(m[e["c"][h]]) + np.abs(m[e["r"][h]]))
    rowb = 4.0 * e["cnt"] * U * np.bincount(e["r"][h], w, minlength=e["n"])
    ob = np.zeros(case["N"]); ob[case["site"][:case["Na"] - 1]] = rowb[2:]
    ratio = (np.abs(ref - o)[written] / ob[written]).max()
    print("oracle against reference, worst |diff| / cancelling-form bound: %.3g" % ratio)
    assert ratio <= 1
    # what the existing 1e-6-of-the-maximum assertion leaves unchecked
    low = written & (ref < 1e-6 * ref.max())
    assert low.sum() == (2600 if case["V"] > 0 else 2602)
    assert np.all(e["x"] <= 0)                                                       # the premise of the bound: one sign per row


def test_bound_covers_any_summation_order(case):
    ref, written, bound = case["ref"]
    e = case["e"]
    h = np.flatnonzero(e["heat"])
    worst = 0.0
    for order in (h[::-1], np.random.default_rng(1).permutation(h), np.random.default_rng(2).permutation(h)):
        s = np.bincount(e["r"][order], e["term"][order], minlength=e["n"])            # (bincount adds in the order given)
        got = np.zeros(case["N"]); got[case["site"][:case["Na"] - 1]] = -s[2:]
        d = np.abs(got - ref)[written]
        assert np.all(d <= bound[written])
        worst = max(worst, (d[bound[written] > 0] / bound[written][bound[written] > 0]).max())
    print("fp64 sums in other orders, worst |diff| / bound: %.3g" % worst)
    assert 0 < worst <= 1


def test_imacro_reference(case):
    val, bound, terms = pr.imacro_reference(case["X"], case["m0"])
    assert len(terms) == 144 and (np.all(terms > 0) or np.all(terms < 0))
    assert (val > 0) == (case["V"] > 0)
    print("I_macro: |ref - oracle| / bound = %.3g, relative %.3g" % (abs(val - case["imacro"]) / bound, abs(val / case["imacro"] - 1)))
    assert abs(val - case["imacro"]) <= bound
    # the shift moves every potential by the same amount: the rule gives the same current from the shifted buffer within the bound of those terms
    val2, bound2, _ = pr.imacro_reference(case["X"], case["m"])
    assert abs(val2 - val) <= bound + bound2


def _caught(case, fault):
    """(out, low): the sites on which the faulty evaluation leaves the bound, and those of them below 1e-6 of the largest power"""
    ref, written, bound = case["ref"]
    got, w2, _ = fault
    out = (np.abs(got - ref) > bound) | (w2 != written)
    return out, out & written & (ref < 1e-6 * ref.max())


def _variant(case, **kw):
    return pr.site_power_reference(case["X"], case["m"], kw.pop("V", case["V"]), case["site"], case["metal"], case["N"], **kw)


def test_reference_resolves_seeded_faults(case):
    """A green comparison means something only if a wrong kernel would leave the bound.  Four faults of the kind the kernels could have, each seeded
    into the reference's own evaluation, each caught on at least one site below 1e-6 of the largest power, where the oracle comparison is blind.

    The two faults of the tunnelling block touch the rows of the tunnelling set only, and those are the hot ones: at +5 V not one of the 400 vacancy
    sites lies below 1e-6 of the largest power (at -3 V two do, and both faults are seeded where they are).  So these two are asserted to leave the
    bound on the sites they touch, and on a site below 1e-6 of the largest wherever they touch one; the other two on such sites at both biases."""
    from devicekmc_amd import params as pm
    ref, written, bound = case["ref"]
    e, Na = case["e"], case["Na"]
    r, c, heat = e["r"], e["c"], e["heat"]
    tun = cmr.site_dist(case["ax"], case["ay"], case["az"], r - 2, c - 2, case["p"].lattice[1], case["p"].lattice[2], 0) >= case["p"].nn_dist
    vac_row = np.zeros(e["n"], dtype=bool); vac_row[2:] = case["ael"][:Na - 1] == pm.VACANCY
    S = np.unique(r[tun])                                            # the tunnelling set, in the order of its ranks
    Sv = S[vac_row[S]]
    assert len(Sv) == 400
    vac_low = ref[case["site"][Sv - 2]] < 1e-6 * ref.max()
    assert vac_low.sum() == (0 if case["V"] > 0 else 2)
    weakest = int(Sv[ref[case["site"][Sv - 2]].argmin()])
    # (1) a vacancy row that misses its tunnelling part: the vacancy row of the smallest power
    assert (heat & tun & (r == weakest)).sum() > 0
    out, low = _caught(case, _variant(case, entries=e, keep=~((r == weakest) & tun)))
    assert out.sum() == 1 and out[case["site"][weakest - 2]]
    assert low.sum() == (1 if vac_low.any() else 0)
    # (2) a 32 x 32 block of the tunnelling set (one sub-block of a tile) that heats the column end where the row end is due and the row end
    # where the column end is: the block of that row against the first 32 ranks
    k = int(np.searchsorted(S, weakest)) // 32
    rows_b, cols_b = S[:32], S[32 * k:32 * k + 32]
    blk = (np.isin(r, rows_b) & np.isin(c, cols_b)) | (np.isin(r, cols_b) & np.isin(c, rows_b))
    blk &= tun & (e["ical"] != 0)
    assert blk.sum() > 64
    out, low = _caught(case, _variant(case, entries=e, heat=np.where(blk, ~heat, heat)))
    assert out.sum() >= 32 and low.sum() == vac_low[np.isin(Sv, cols_b)].sum() and low.any() == vac_low.any()
    # (3) the predicate with the sign of Vd flipped
    assert _caught(case, _variant(case, V=-case["V"]))[1].sum() > 2000
    # (4) the last atom row dropped.  (The system's very last row belongs to a contact metal atom, which no form writes: the last row that IS
    # written is the one a short grid loses first.)
    nm = np.flatnonzero(~case["metal"][:Na - 1]) + 2
    last = int(nm[-1])
    out, low = _caught(case, _variant(case, entries=e, rows=np.arange(2, last)))
    assert low.sum() == 1 and low[case["site"][last - 2]]
    # ... and the entries themselves stand clear of the bound of their row: 99 % of the heating entries of written rows, one in every row at least
    val, mag, num = pr.row_sums(e)
    rowb = 4.0 * e["cnt"] * U * mag
    wr = np.zeros(e["n"], dtype=bool); wr[nm] = True
    sel = heat & wr[r]
    clear = np.abs(e["term"][sel]) > 2.0 * rowb[r[sel]]
    share = clear.mean()
    print("heating entries above twice their row's bound: %.2f %%" % (100 * share))
    assert share >= 0.99
    assert np.all(np.bincount(r[sel][clear], minlength=e["n"])[nm] > 0) and len(nm) == 3000


def temperature_grid():
    """(mode, P, T0, arguments of temperature_reference): powers, start temperatures and steps from far too short to matter to the steady state"""
    from devicekmc_amd import params as pm
    p = pm.KMCParameters()
    Cth = p.A * p.t_ox * p.c_p * 1e6
    a = -p.dissipation_constant / Cth * p.small_step + 1; b = p.dissipation_constant / Cth * p.small_step * p.background_temp
    for P, T0 in itertools.product((0.0, 8.757671252262462e-16, 1e-11, 3e-11), (300.0, 812.5)):
        for t in (1e-13, 1e-9, 1e-7, 1e-6, 1e-3):
            yield 0, P, T0, dict(event_time=t, dissipation_constant=p.dissipation_constant, C=Cth)
        for s in (0, 1, 10000.5, 1e9, 2e9):
            yield 1, P, T0, dict(a_coeff=a, b_coeff=b, number_steps=s, C_thermal=Cth, small_step=p.small_step)


def test_closed_forms_in_fp64_stay_within_the_bound():
    worst = {0: 0.0, 1: 0.0}
    moved = 0
    for mode, P, T0, kw in temperature_grid():
        T, bound, steady = pr.temperature_reference(mode, P, T0, **kw)
        got = pr.temperature_fp64(mode, P, T0, **kw)
        assert abs(got - T) <= bound, (mode, P, T0, kw, got, T, bound)
        worst[mode] = max(worst[mode], abs(got - T) / bound)
        moved += abs(T - T0) > 1e6 * bound
    print("fp64 closed forms, worst |diff| / bound: mode 0 %.3g, mode 1 %.3g" % (worst[0], worst[1]))
    assert moved > 40                                                # the grid is not all steps too short to matter
    # the case the issue quotes: 1e-11 W for 1e-7 s is a rise of about 14 K against a bound of about 1.2e-12 K
    from devicekmc_amd import params as pm
    p = pm.KMCParameters()
    T, bound, _ = pr.temperature_reference(0, 1e-11, 300.0, event_time=1e-7, dissipation_constant=p.dissipation_constant, C=p.A * p.t_ox * p.c_p * 1e6)
    assert 13.0 < T - 300.0 < 15.0 and bound < 1.3e-12


def test_power_sum_bound():
    rng = np.random.default_rng(3)
    p = 10.0 ** rng.uniform(-24, -11, 100001)
    exact = math.fsum(p)
    for order in (p, p[::-1], np.sort(p), np.sort(p)[::-1]):
        s = 0.0
        for v in order[:20000]:
            s += v
        assert abs(s - math.fsum(order[:20000])) <= pr.power_sum_bound(order[:20000])
        assert abs(float(np.sum(order)) - exact) <= pr.power_sum_bound(p)
