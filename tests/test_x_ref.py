"""The longdouble reference of X (tests/x_ref.py) pinned before it is trusted: against the CPU oracle's assemble_X on every synthetic case of
tests/x_cases.py and on the shipped 2.5 nm cell, against mpmath at 40 digits on sampled entries, and against the case table.  No GPU.

The value bound is a measurement: R_KIND (x_cases.py) is the oracle's largest relative deviation from the reference per kind of entry, float64
against longdouble with the kernel's formulas on both sides; this module asserts that the oracle stays inside it, and the GPU tests use 8 R."""
import numpy as np
import pytest

import x_cases
import x_ref

LD = np.longdouble
U = 2.0 ** -53
_cache = {}


def _cell(cell_2p5):
    from devicekmc_amd import params as pm
    p = pm.KMCParameters()
    return cell_2p5, p, 5.0, None, (828, 928)


def _pair(name, cell_2p5):
    """(oracle X, reference, p, expected counts) of a case, built once"""
    if name not in _cache:
        from oracle import oracle as oc
        s, p, Vd, cb, counts = _cell(cell_2p5) if name == "cell_2p5" else x_cases.make_case(name)
        o = oc.OracleKMC(s.element, s.x, s.y, s.z, p)
        if cb is None:
            o.set_laplace_potential(Vd); cb = o.CB_edge.copy()
        else:
            o.CB_edge[:] = cb
        o.update_charge()
        X = o.assemble_X()
        ref = x_cases.reference_of(x_ref, s, p, cb, o.element, o.charge, o.neigh)
        _cache[name] = (X, ref, p, counts, s, cb)
    return _cache[name]


ALL = x_cases.NAMES + ["cell_2p5"]


@pytest.mark.parametrize("name", ALL)
def test_reference_against_the_oracle(name, cell_2p5):
    """Pattern exact; nM and ns of the table; direct, boundary and row-0/1 entries equal; tunnelling values within R_KIND per kind; the diagonal
    within sum R |t| + n_i u sum |off| (the oracle adds its n_i - 1 off-diagonals one by one and subtracts once)."""
    X, ref, p, (nM, ns), _, _ = _pair(name, cell_2p5)
    assert (ref["nM"], ref["ns"]) == (nM, ns)
    assert np.array_equal(ref["rp"], X["row_ptr"]) and np.array_equal(ref["ci"], X["col"])
    v, d, k = ref["val"], X["data"].astype(LD), ref["kind"]
    exact = (k == 0) | (k == 3)
    assert np.array_equal(d[exact], v[exact])
    err = np.abs(d - v)
    bound = np.zeros(len(v), dtype=LD)
    for kind in (1, 2):
        m = k == kind
        if m.any():
            rel = float((err[m] / np.abs(v[m])).max())
            print("%s kind %d: %d entries, max rel %.3e (R %.0e)" % (name, kind, m.sum(), rel, x_cases.R_KIND[kind]))
            assert rel <= x_cases.R_KIND[kind]
            bound[m] = x_cases.R_KIND[kind] * np.abs(v[m])
    assert np.all(v[(k == 1) | (k == 2)] < 0)
    rowb = np.zeros(len(ref["rp"]) - 1, dtype=LD); np.add.at(rowb, ref["row"], bound)
    cnt = np.diff(ref["rp"])
    dp = ref["diag_pos"]
    assert np.all(err[dp] <= rowb + cnt * U * ref["offabs"])
    # rows without boundary terms sum to zero: columns 0 / 1 absent and no ground term
    has_pre = np.zeros(len(cnt), dtype=bool); has_pre[ref["row"][k == 0]] = True
    free = ~has_pre; free[:2] = False; free[2:] &= ~ref["ground_term"][:len(cnt) - 2]
    assert free.sum() > 0
    for data, eps in ((v, 2.0 ** -63), (d, U)):
        rs = np.zeros(len(cnt), dtype=LD); np.add.at(rs, ref["row"], data)
        assert np.all(np.abs(rs[free]) <= (cnt[free] + 1) * eps * ref["offabs"][free])


@pytest.mark.parametrize("name", ALL)
def test_tunnelling_block_is_symmetric(name, cell_2p5):
    _, ref, _, _, _, _ = _pair(name, cell_2p5)
    T = ref["T"]
    assert np.array_equal(T, T.T) and np.all(np.diag(T) == 0) and np.all(T <= 0)
    assert np.array_equal(ref["pred"], ref["pred"].T) and np.array_equal(T != 0, ref["pred"])
    # the CSR holds exactly the tunnelling entries of T whose pair also passes the narrow window
    k = ref["kind"]
    assert ((k == 1) | (k == 2)).sum() <= (T != 0).sum()


def test_metals_first_order():
    _, ref, p, _, _, _ = _pair("n64_v257", None)
    S, Smf, nM = ref["S_atom"], ref["S_metals_first"], ref["nM"]
    assert np.all(np.diff(S) > 0) and np.array_equal(np.sort(Smf), S)
    assert ref["metal"][Smf[:nM]].all() and not ref["metal"][Smf[nM:]].any()
    assert np.all(np.diff(Smf[:nM]) > 0) and np.all(np.diff(Smf[nM:]) > 0)


def _mp_entry(mp, kind, levels, xa, xb, cba, cbb, p, pbc=False):
    """wkb_T in mpmath from the float64 inputs; the level count is the float64 decision of the reference"""
    f = lambda v: mp.mpf(float(v))
    d = mp.sqrt(sum((f(xb[i]) - f(xa[i])) ** 2 for i in range(3))) * f(1e-10)
    drop = abs(f(cba) - f(cbb))
    prefac = -(mp.sqrt(2 * f(p.m_e)) / f(x_ref.HBAR)) * (mp.mpf(2) / 3)
    QV0 = f(x_ref.Q) * f(p.V0)
    p15 = lambda e: e * mp.sqrt(e)
    if kind == 2:
        E1, E2 = QV0, QV0 - drop
        c = prefac * (d / abs(E1 - E2))
        return mp.exp(c * (p15(E1) - p15(E2))) if E2 > 0 else mp.exp(c * p15(E1))
    c = prefac * (d / drop)
    T = mp.mpf(0)
    for ivk in x_ref._IV[:levels]:
        E1 = QV0 + f(ivk); E2 = E1 - drop
        T += mp.exp(c * (p15(E1) - p15(E2))) if E2 > 0 else mp.exp(c * p15(E1))
    return T


def test_sampled_entries_against_mpmath():
    """Twenty entries, ten of each kind, spread over the range of the CB difference so that both branches on the sign of E2 are met (kind 2: E2 > 0
    and E2 < 0; kind 1: integrals with levels on both sides): the longdouble value against mpmath at 40 digits to 1e-17 relative."""
    import mpmath as mp
    mp.mp.dps = 40
    _, ref, p, _, s, cb = _pair("n303_v5", None)
    S = ref["S_atom"]; site = ref["atom_site"][S]
    T, kT, lv, br = ref["T"], ref["kindT"], ref["levels"], ref["branch"]
    seen = set(); worst = 0.0
    for kind in (1, 2):
        I, J = np.nonzero(np.triu(kT == kind, 1))
        drop = np.abs(cb[site[I]] - cb[site[J]])
        pick = np.argsort(drop, kind="stable")[np.linspace(0, len(I) - 1, 10).astype(int)]
        for e in pick:
            i, j = I[e], J[e]
            a, b = site[i], site[j]
            want = _mp_entry(mp, kind, int(lv[i, j]), (s.x[a], s.y[a], s.z[a]), (s.x[b], s.y[b], s.z[b]), cb[a], cb[b], p)
            mant, ex = np.frexp(-T[i, j])                              # exact: the 64-bit significand as an integer
            got = mp.mpf(int(mant * LD(2) ** 64)) * mp.mpf(2) ** (int(ex) - 64)
            rel = float(abs(got / want - 1))
            worst = max(worst, rel); seen.add((kind, int(br[i, j])))
            print("kind %d levels %3d branch %d: %.6e rel %.2e" % (kind, lv[i, j], br[i, j], float(want), rel))
    assert {(2, 1), (2, 2)} <= seen and any(k == 1 and b & 1 for k, b in seen) and any(k == 1 and b & 2 for k, b in seen), seen
    assert worst <= 1e-17, worst


def test_metals_only_entries_are_small_after_scaling():
    """(64, 2, 0): every scaled entry |t_ij| / sqrt(d_i d_j) is below 1e-4, which is what makes every tile dead under dkmc_set_x_tile_drop(1e-4)"""
    _, ref, _, _, _, _ = _pair("n64_v0", None)
    d = ref["val"][ref["diag_pos"]][ref["S_atom"] + 2].astype(np.float64)
    sc = np.abs(ref["T"].astype(np.float64)) / np.sqrt(np.outer(d, d))
    print("metals only: largest scaled entry %.3e" % sc.max())
    assert np.all(d > 0) and sc.max() < 1e-4


def test_census_of_a_hand_made_predicate():
    """x_ref.census on a predicate whose cells are known: a pair on the diagonal sub-block's upper side, one across a window edge, one below the
    diagonal only (no bit)."""
    ns = 300
    pred = np.zeros((ns, ns), dtype=bool)
    for r, c in ((0, 1), (31, 256), (40, 299), (290, 280)):
        pred[r, c] = True
    masks, up = x_ref.census(pred | pred.T)
    want = np.zeros((10, 2), dtype=np.int64)
    want[0, 0] = 1; want[0, 1] = 1; want[1, 1] = 1 << 1; want[8, 1] = 1 << 1          # (280, 290): row block 8, window 1, sub-block (290 - 256) // 32
    assert np.array_equal(masks, want) and up.sum() == 4


def test_an_inclusive_level_loop_is_seen():
    """The level loop of wkb_T run with iv <= drop (a seeded fault) moves the contact->trap values of the threshold case, whose CB differences sit
    on the level grid, far outside 8 R; elsewhere it changes nothing (no difference equals a level)."""
    X, ref, p, _, s, cb = _pair("threshold", None)
    from oracle import oracle as oc
    o = oc.OracleKMC(s.element, s.x, s.y, s.z, p); o.update_charge()
    bad = x_cases.reference_of(x_ref, s, p, cb, o.element, o.charge, o.neigh, inclusive_levels=True)
    m = ref["kind"] == 1
    rel = np.abs(bad["val"][m] / ref["val"][m] - 1).astype(np.float64)
    print("inclusive level loop: %d of %d contact->trap entries move, by up to %.2e" % ((rel > 8 * x_cases.R_KIND[1]).sum(), m.sum(), rel.max()))
    assert (rel > 1e-3).sum() > 100
