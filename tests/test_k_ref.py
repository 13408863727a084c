"""The longdouble reference of K (tests/k_ref.py) pinned before it is trusted: against the CPU oracle's patterns, assembly and converged CG on every
synthetic case of tests/k_cases.py and on the shipped 2.5 nm cell, and the cases themselves against the shape claims of their table.  No GPU.

The oracle adds a row's n terms one by one in float64: its diagonal and right-hand side lie within (n + 2) 2^-53 of the reference, relative (all
terms of a diagonal have one sign; the right-hand side is compared relative to |kl VL| + |kr VR|).  Off-diagonal values are +-high_G, +-low_G or
absent and equal bit for bit.  Every check prints its worst figure for DESIGN.md section 2."""
import numpy as np
import pytest

import k_cases
import k_ref

LD = np.longdouble
U = 2.0 ** -53
TOL = 1e-12
_cache = {}
ALL = k_cases.SMALL + ["L", "cell_2p5"]


def _oracle(name, cell_2p5):
    """(oracle with charges updated, p) of a case, built once"""
    if name not in _cache:
        from devicekmc_amd import params as pm
        from oracle import oracle as oc
        s, p = (cell_2p5, pm.KMCParameters()) if name == "cell_2p5" else k_cases.make_case(name)
        o = oc.OracleKMC(s.element, s.x, s.y, s.z, p)
        o.update_charge()
        _cache[name] = (o, p)
    return _cache[name]


def _contacts(rule, Vd):
    return (-Vd / 2, Vd / 2) if rule == 0 else (Vd / 2, -Vd / 2)


@pytest.mark.parametrize("name", ALL)
def test_charge_rule_against_the_oracle(name, cell_2p5):
    o, p = _oracle(name, cell_2p5)
    assert np.array_equal(k_ref.charges(o.neigh, o.element, np.zeros(o.N, dtype=np.int32), p.metals), o.charge)


@pytest.mark.parametrize("name", ALL)
def test_patterns_against_the_oracle(name, cell_2p5):
    o, p = _oracle(name, cell_2p5)
    nl, m, pats = o.initialize_sparsity()
    (P, Pl, Pr), _ = k_ref.patterns(o.neigh, p.num_atoms_first_layer)
    for (rp, ci), (orp, oci) in zip((P, Pl, Pr), pats):
        assert np.array_equal(rp, orp) and np.array_equal(ci, oci)
    rows = np.repeat(np.arange(m), np.diff(P[0]))
    assert (np.bincount(rows[P[1] == rows], minlength=m) == 1).all() and (np.diff(P[1])[np.diff(rows) == 0] > 0).all()


@pytest.mark.parametrize("rule", [0, 1, 2])
@pytest.mark.parametrize("name", ALL)
def test_assembly_against_the_oracle(name, rule, cell_2p5):
    o, p = _oracle(name, cell_2p5)
    worst = [0.0, 0.0]
    for Vd in k_cases.biases(name):
        VL, VR = _contacts(rule, Vd)
        S = k_cases.reference_of(k_ref, p, o.neigh, o.element, o.charge, Vd, rule)
        o._K = None
        nl, m, ((rp, ci), (lrp, lci), (rrp, rci)) = o.initialize_sparsity()
        import ctypes as C
        from oracle.oracle import _p, lib
        data = np.zeros(len(ci)); rhs = np.zeros(m)
        lib().okmc_k_assemble(o.N, nl, nl, _p(o.element), _p(o.charge), _p(o.metals), len(o.metals), C.c_double(p.high_G), C.c_double(p.low_G), rule,
                              _p(rp), _p(ci), _p(lrp), _p(lci), _p(rrp), _p(rci), C.c_double(VL), C.c_double(VR), _p(data), _p(rhs))
        offd = S["ci"] != S["rows"]
        assert np.array_equal(data[offd].astype(LD), S["val"][offd])
        assert set(np.unique(data[offd])) <= {0.0, -p.high_G, -p.low_G}
        d = data[~offd]
        derr = np.abs(d.astype(LD) - S["diag"]) / S["diag"]
        assert np.all(derr <= (S["nterm"] + 2) * U)
        rerr = np.abs(rhs.astype(LD) - S["rhs"])
        rb = (S["nrhs"] + 2) * U * S["rhs_abs"]
        assert np.all(rerr <= rb)
        if rule == 2:
            assert np.all(d[S["identity"]] == 1.0) and np.all(rhs[S["identity"]] == 0.0)
        worst[0] = max(worst[0], float((derr / ((S["nterm"] + 2) * U)).max()))
        worst[1] = max(worst[1], float((rerr[rb > 0] / rb[rb > 0]).max()) if (rb > 0).any() else 0.0)
    print("k-ref assembly %-8s rule %d: diag %.3f / 1, rhs %.3f / 1 of the bound" % (name, rule, worst[0], worst[1]))


@pytest.mark.parametrize("rule", [0, 1, 2])
@pytest.mark.parametrize("name", k_cases.SMALL + ["cell_2p5"])
def test_converged_oracle_solve_meets_the_reference(name, rule, cell_2p5):
    """OracleKMC._solve_K at 1e-12 from zero: the residual of its solution in the reference's K is within 10 tol; its distance from the refined
    LU solution is printed."""
    o, p = _oracle(name, cell_2p5)
    n = p.num_atoms_first_layer
    for Vd in k_cases.biases(name):
        VL, VR = _contacts(rule, Vd)
        S = k_cases.reference_of(k_ref, p, o.neigh, o.element, o.charge, Vd, rule)
        field = np.zeros(o.N)
        o._K = None
        it, rr = o._solve_K(field, VL, VR, rule, TOL)
        y = field[n:o.N - n]
        res = k_ref.scaled_residual(S, y)
        yref, res0 = k_ref.solve(S)
        dy = float(np.abs(y.astype(LD) - yref).max())
        print("k-ref solve %-8s rule %d Vd %+.0f: oracle %4d iterations, residual / tol %.3f, max |y - y_ref| %.2e V, reference residual %.1e"
              % (name, rule, Vd, it, res / TOL, dy, res0))
        assert res <= 10 * TOL
        if Vd == 0.0:
            assert it == 0 and not y.any() and not yref.any()
        else:
            assert it > 0


# ---- the cases against their table ----------------------------------------------------------------------------------------------------------------
def _hist(name, cell_2p5=None):
    o, p = _oracle(name, cell_2p5)
    S = {r: k_cases.reference_of(k_ref, p, o.neigh, o.element, o.charge, 5.0, r) for r in (0, 1, 2)}
    return o, p, S


@pytest.mark.parametrize("name", k_cases.SMALL + ["L"])
def test_case_shapes(name):
    o, p, S = _hist(name)
    ny, nz, nc, nox, nn_dist, n_first, nV, pbc = k_cases.CASES[name]
    od = S[0]["offdiag"]
    assert o.N == ny * nz * (2 * nc + nox) + 10 and S[0]["m"] == o.N - 2 * n_first
    assert not (S[0]["diag"] == 0).any() and not (S[1]["diag"] == 0).any()
    assert not S[0]["identity"].any() and not S[1]["identity"].any()
    assert S[2]["identity"].sum() == k_cases.IDENTITY_ROWS[name]
    want = {"a": (3, 13), "c": (10, 36), "d": (19, 85)}
    if name in want:
        assert (od.min(), od.max()) == want[name]
    if name in ("a", "b", "f", "g63", "g65", "L"):
        assert od.max() <= 32 and S[0]["m"] % 64 != 0
    if name == "a":
        assert (o.N, S[0]["m"], o.nn) == (1290, 1162, 13) and S[0]["m"] == 18 * 64 + 10
    if name == "b":
        oa, _, Sa = _hist("a")
        assert len(S[0]["ci"]) > len(Sa[0]["ci"])                               # wrapped links
    if name == "c":
        assert S[0]["m"] == 1034 and (od == 32).sum() == 167 and (od > 32).sum() == 68 and od.max() <= 64
    if name == "d":
        assert (o.N, S[0]["m"]) == (2010, 1610) and (od > 64).sum() == 796
        rows = np.diff(S[0]["rp"])
        assert rows.max() == 86 and (rows > 32).any() and (rows > 64).any()       # second and third pass of the 32-entry loop of the CSR product
    if name == "e":
        both = (S[0]["kl"] > 0) & (S[0]["kr"] > 0)
        assert both.sum() == ny * nz and (np.abs(S[0]["rhs"][both]) < S[0]["rhs_abs"][both]).all()
    if name in ("g63", "g65"):
        assert n_first % (ny * nz) != 0
    if name == "L":
        m = S[0]["m"]
        R = (-(-m // 256) + 63) // 64 * 64
        assert (o.N, m, R) == (140618, 135210, 576) and m > 131072 and 4 * ny * nz <= 14336


def test_case_f_reaches_every_branch_of_the_rules():
    from devicekmc_amd import params as pm
    o, p, S = _hist("f")
    el, q, n = o.element, o.charge, p.num_atoms_first_layer
    s0 = S[0]
    i, j = n + s0["rows"], n + s0["ci"]
    off = i != j
    metal = np.isin(el, p.metals)
    cv = (el == pm.VACANCY) & (q == 0)
    vac2 = (el == pm.VACANCY) & (q == 2)
    high = s0["cls"] == k_ref.HIGH
    assert (off & cv[i] & cv[j]).sum() >= 2 and high[off & cv[i] & cv[j]].all()             # two adjacent neutral vacancies: high
    assert (off & vac2[i] & cv[j]).any() and not high[off & vac2[i] & cv[j]].any()          # a +2 vacancy next to a neutral one: low
    assert (off & cv[i] & metal[j]).any() and not high[off & cv[i] & metal[j]].any()        # a neutral vacancy next to a metal: low under rule 0
    assert (off & metal[i] & metal[j]).any() and (off & metal[i] & ~metal[j]).any()
    assert (off & (el[i] == pm.N_EL)).any() and set(p.metals) >= {pm.N_EL, pm.Ti_EL}
    od = el == pm.OXYGEN_DEFECT
    assert (od & (q == -2)).any() and (od & (q == 0)).sum() >= 2
    # rule 2: an interstitial inside a contact (an entry the contact sums skip) and an interstitial row next to a contact (a row they cut)
    s1, s2 = S[1], S[2]
    inter = (el == pm.DEFECT) | (el == pm.OXYGEN_DEFECT)
    lrows = np.repeat(np.arange(s2["m"]), np.diff(s2["lrp"]))
    skipped = inter[s2["lci"]] & ~inter[n + lrows]
    cut = inter[n + lrows]
    assert skipped.any() and cut.any()
    assert (s2["kl"] < s1["kl"]).sum() >= 2 and (s2["cls_left"] == k_ref.NOLINK).sum() == (skipped | cut).sum()
