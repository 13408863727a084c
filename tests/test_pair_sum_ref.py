"""Pins tests/pair_sum_ref.py, the reference of tests/test_gpu_pair_sum_boxes.py, and the inputs of its cases -- no GPU.  For every case: v_all
against the oracle's okmc_poisson_gridless within 1e-12 of the largest potential (the project's bound for that comparison) and, on 8 sites, against
a 40-digit mpmath evaluation within 1e-14 of the site's sum of magnitudes; no pair closer than 1e-9 (relative, in d2) to the cut-off, so that the
kernels' FMA-contracted d2 cannot classify a pair differently; no charged site within 1e-3 A of another site; and pair_grid_ref gives exactly the
column grid the case was built to reach."""
import ctypes as C

import numpy as np
import pytest

import pair_sum_ref as R


def _oracle_sum(c, pbc, q):
    from oracle import oracle as oc
    want = np.zeros(c.N)
    lat = np.asarray(c.lattice, dtype=np.float64)
    x, y, z = (np.ascontiguousarray(a, dtype=np.float64) for a in (c.x, c.y, c.z))
    qq = np.ascontiguousarray(q, dtype=np.int32)
    oc.lib().okmc_poisson_gridless(c.N, oc._p(x), oc._p(y), oc._p(z), oc._p(lat), int(pbc), C.c_double(c.sigma), C.c_double(R.K), oc._p(qq), oc._p(want))
    return want


def _steps(name):
    return range(2 if name == "threshold" else 1)          # threshold's third step repeats its first


@pytest.mark.parametrize("name,pbc", R.RUNS)
def test_v_all_against_the_oracle(name, pbc):
    c = R.case(name)
    for k in _steps(name):
        ref = R.reference(name, pbc, k)
        want = _oracle_sum(c, pbc, c.steps[k].q)
        scale = np.abs(ref.v_all).max()
        err = np.abs(ref.v_all - want).max()
        print("%s pbc %d step %d: max |ref - oracle| = %.2e of the largest potential" % (name, pbc, k, err / scale))
        assert scale > 0 and err <= 1e-12 * scale


@pytest.mark.parametrize("name,pbc", R.RUNS)
def test_v_all_against_40_digits(name, pbc):
    mp = pytest.importorskip("mpmath")
    c = R.case(name)
    ref = R.reference(name, pbc)
    q = c.steps[0].q
    cj = np.flatnonzero(q)
    assert len(c.probes) == 8 and c.probes[0] == 0 and c.probes[1] == c.N - 1 and len(set(c.probes.tolist())) == 8
    with mp.workdps(40):
        f = mp.mpf
        ly, lz, s2, kq, ang = f(c.lattice[1]), f(c.lattice[2]), f(c.sigma) * mp.sqrt(2), f(R.K) * f(R.Q), f(1e-10)
        rnd = lambda v: mp.sign(v) * mp.floor(abs(v) + f(0.5))          # C round()
        worst = 0.0
        for i in c.probes:
            tot, mag = f(0), f(0)
            for j in cj:
                if j == i:
                    continue
                dx, dy, dz = f(c.x[i]) - f(c.x[j]), f(c.y[i]) - f(c.y[j]), f(c.z[i]) - f(c.z[j])
                if pbc:
                    fy, fz = dy / ly, dz / lz
                    dy, dz = (fy - rnd(fy)) * ly, (fz - rnd(fz)) * lz
                r = ang * mp.sqrt(dx * dx + dy * dy + dz * dz)
                t = int(q[j]) * mp.erfc(r / s2) * kq / r
                tot += t; mag += abs(t)
            err = abs(f(float(ref.v_all[i])) + f(float(ref.v_all[i] - np.longdouble(float(ref.v_all[i])))) - tot)
            assert mag > 0 and err <= f(1e-14) * mag, (name, pbc, int(i), float(err / mag))
            worst = max(worst, float(err / mag))
    print("%s pbc %d: max |ref - 40 digits| = %.2e of the site's sum of magnitudes" % (name, pbc, worst))


@pytest.mark.parametrize("name,pbc", R.RUNS)
def test_inputs_keep_clear_of_the_cutoff_and_of_each_other(name, pbc):
    for k in _steps(name):
        ref = R.reference(name, pbc, k)
        assert ref.margin >= 1e-9, (name, pbc, k, ref.margin)
        assert ref.d2_min >= 1e-6, (name, pbc, k, ref.d2_min)
        assert np.array_equal(ref.n_in == 0, ref.abs_in == 0)


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_reaches_its_branch(name):
    """The grid row of every case, its sizes, and the properties its row of the table names."""
    c = R.case(name)
    assert c.name == name and c.N <= 20000 and c.pbcs == tuple(p for n, p in R.RUNS if n == name)
    for s in c.steps:
        nq = int((s.q != 0).sum())
        assert nq <= 2000 and set(np.unique(s.q[s.q != 0])) == {-2, -1, 1, 2}
        assert R.pair_grid_ref(c.lattice, c.sigma, R.XCUT, nq) == s.grid, (name, nq)
    ny, nz, ry, rz, nx, use = c.steps[0].grid
    q = c.steps[0].q
    rc = R.XCUT * c.sigma * np.sqrt(2.0) * 1e10
    col = R.column_of(c.y, c.z, c.lattice, ny, nz, 0)
    per_col = np.bincount(col, minlength=ny * nz)
    charged_per_col = np.bincount(col[q != 0], minlength=ny * nz)
    if name in ("rect", "rect_T"):
        assert ny != nz and ry == rz == 2 and ny >= 5 and nz >= 5
    if name == "rect_T":
        r = R.case("rect")
        assert np.array_equal(c.y, r.z) and np.array_equal(c.z, r.y) and np.array_equal(c.x, r.x) and np.array_equal(q, r.steps[0].q)
        assert c.lattice == (r.lattice[0], r.lattice[2], r.lattice[1]) and (ny, nz) == (r.steps[0].grid[1], r.steps[0].grid[0])
    if name == "narrow_z":
        assert nz < 2 * rz + 1 and ny >= 2 * ry + 1
    if name == "sliver_z":
        assert c.lattice[2] < rc / 2 and (nz, rz) == (1, 3)
    if name == "both_narrow":
        nq = int((q != 0).sum())
        assert use == 0 and nq >= R.PW_MIN_CHARGED and 2 * 256 < nq < 3 * 256          # three LDS tiles of k_pairwise, the last one partial
    if name == "clamp_y":
        assert ny == R.PW_MAXDIM and 2.0 * c.lattice[1] / rc > R.PW_MAXDIM and ry == 2
    if name == "full_grid":
        assert ny * nz == R.PW_MAXDIM ** 2 and c.lattice[1] / ny > rc and ry == rz == 1
        assert 0 < per_col.max() < R.PW_SITES                                          # every chunk is partial
    if name == "holes":
        assert per_col[0] == 0 and per_col[-1] == 0 and (per_col[1:-1] == 0).sum() > 20
        assert (per_col == 64).sum() >= 1 and (per_col == 65).sum() >= 1
        occupied = per_col > 0
        assert (occupied & (charged_per_col == 0)).sum() == occupied.sum() // 4
    if name == "outside":
        lx, ly, lz = c.lattice
        lateral = (c.y < 0) | (c.y > ly) | (c.z < 0) | (c.z > lz)
        assert lateral.sum() == c.N // 20 and ((c.x < 0) | (c.x > lx)).sum() == c.N // 20
        assert (c.y < -ly).any() and (c.y > 2 * ly).any() and (c.z < -lz).any() and (c.z > 2 * lz).any()
        assert (c.y == 0.0).sum() == 2 and (c.y == ly).sum() == 2 and sum(int((c.y == m * (ly / ny)).sum()) for m in range(1, ny)) == 16
        assert (q[lateral] != 0).any() and (q[(c.x < 0) | (c.x > lx)] != 0).any()
    if name == "thin_x":
        assert nx == 1
    if name == "long_x":
        assert nx == R.PW_MAXX and 4.0 * c.lattice[0] / rc > R.PW_MAXX and c.tested_below == 0.6
        assert ((c.x < 10) | (c.x > 140)).all() and (c.x < 10).any() and (c.x > 140).any()
    if name == "big_segment":
        assert nx == 1 and per_col.max() > R.PW_SORTCAP
    if name == "physical":
        assert c.sigma == 3.5e-10 and ny != nz
    if name == "threshold":
        r = R.case("rect")
        assert np.array_equal(c.x, r.x) and np.array_equal(c.y, r.y) and np.array_equal(c.z, r.z)
        assert [int((s.q != 0).sum()) for s in c.steps] == [512, 511, 512] and [s.grid[5] for s in c.steps] == [1, 0, 1]
        assert np.array_equal(c.steps[0].q, c.steps[2].q)


def test_pair_sum_ref_on_a_hand_case():
    """Three sites on a line, 5 A apart, two charged: every quantity of the reference from its definition; then one pair across the periodic face."""
    from math import erfc, sqrt
    x, y, z = np.array([0.0, 3.0, 6.0]), np.zeros(3), np.array([0.0, 4.0, 8.0])
    q = np.array([2, -1, 0], dtype=np.int32)
    sigma, k = 1e-10, R.K
    t = lambda qq, r: qq * erfc(r * 1e-10 / (sigma * sqrt(2.0))) * k * R.Q / (r * 1e-10)
    ref = R.pair_sum_ref(x, y, z, (10.0, 10.0, 10.0), 0, sigma, k, q, 4.0)          # cut2 = 32 A^2: the 5 A pairs inside, the 10 A pair outside
    assert ref.n_in.tolist() == [1, 1, 1]
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    assert np.allclose(f64(ref.v_all), [t(-1, 5.0), t(2, 5.0), t(2, 10.0) + t(-1, 5.0)], rtol=1e-14, atol=0)
    assert np.allclose(f64(ref.v_in), [t(-1, 5.0), t(2, 5.0), t(-1, 5.0)], rtol=1e-14, atol=0)
    assert np.allclose(f64(ref.abs_in), [t(1, 5.0), t(2, 5.0), t(1, 5.0)], rtol=1e-14, atol=0)
    assert abs(ref.margin - (1.0 - 25.0 / R.cut2_of(sigma, 4.0))) < 1e-15 and ref.d2_min == 25.0
    ref = R.pair_sum_ref(x, y, z, (10.0, 10.0, 10.0), 0, sigma, k, q, 3.0)          # cut2 = 18 A^2: no pair inside
    assert ref.n_in.tolist() == [0, 0, 0] and not ref.v_in.any() and not ref.abs_in.any() and ref.v_all.all()
    x, y, z, q = np.zeros(2), np.array([1.0, 11.0]), np.zeros(2), np.array([1, 1], dtype=np.int32)
    for pbc, d in ((0, 10.0), (1, 2.0)):                                               # ly = 12: 2 A apart through the face
        ref = R.pair_sum_ref(x, y, z, (10.0, 12.0, 10.0), pbc, sigma, k, q, 4.0)
        assert ref.n_in.tolist() == [pbc, pbc] and abs(ref.d2_min - d * d) < 1e-12
        assert np.allclose(f64(ref.v_all), [t(1, d), t(1, d)], rtol=1e-13, atol=0)
