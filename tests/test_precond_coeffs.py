"""Coefficients of the split polynomial preconditioner L = p(N) (csrc/xtb_precond.h: xtb_poly_coeffs, through dkmc_xtb_poly_coeffs) against a 50-digit
reference: p is the Chebyshev interpolant of degree d of f(x) = (1 - x)^(-1/2) on [-1, 1 - delta], delta = min(0.5, 1.6 / d^2), in the monomial basis.
The block loop only sees "another SPD operator", so a wrong coefficient shows up as more sweeps at most; this pins p itself (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest

import mpmath
mp = mpmath.mp

DEGREES = list(range(1, 17))
GRID = 801                           # points of the dense grid on [-1, 1]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from devicekmc_amd import lib as L
    return L


def _library_coeffs(lib, d):
    pc = np.full(17, np.nan)
    lib.check(lib.load().dkmc_xtb_poly_coeffs(d, pc.ctypes.data_as(C.POINTER(C.c_double))))
    assert np.all(np.isfinite(pc[:d + 1])) and np.all(np.isnan(pc[d + 1:])), pc        # exactly d + 1 coefficients written
    return pc[:d + 1]


def _nodes(d, delta):
    a, b = mp.mpf(-1), 1 - mp.mpf(delta)
    n = d + 1
    return [(b - a) / 2 * mp.cos(mp.pi * (k + mp.mpf(1) / 2) / n) + (b + a) / 2 for k in range(n)]


def _f(x):
    return 1 / mp.sqrt(1 - x)


def _reference(d, delta=None):
    """Monomial coefficients (mpf, 50 digits) of the degree-d interpolant of f at the d + 1 Chebyshev nodes of [-1, 1 - delta]."""
    with mp.workdps(50):
        delta = min(mp.mpf("0.5"), mp.mpf("1.6") / d ** 2) if delta is None else mp.mpf(delta)
        xs = _nodes(d, delta)
        V = mp.matrix([[x ** j for j in range(d + 1)] for x in xs])
        c = mp.lu_solve(V, mp.matrix([_f(x) for x in xs]))
        return [c[j] for j in range(d + 1)]


def _horner(c, x):
    acc = mp.mpf(0)
    for cj in reversed(c):
        acc = acc * x + cj
    return acc


def _grid():
    return [mp.mpf(-1) + 2 * mp.mpf(i) / (GRID - 1) for i in range(GRID)]


def _value_error(pc, ref):
    """max over the grid |p(x) - ref(x)| / sum |c_j| (the library's double coefficients evaluated exactly; ref may be of another degree)."""
    with mp.workdps(50):
        c = [mp.mpf(float(v)) for v in pc]
        scale = sum(abs(v) for v in c)
        return float(max(abs(_horner(c, x) - _horner(ref, x)) for x in _grid()) / scale)


# What the float64 coefficient transformation can reach: the monomial form of a degree-16 Chebyshev sum cancels terms of up to |c| ~ 4.7e3;
# its values still agree with the exact interpolant to within 8e-16 of sum |c_j| (d = 1 ... 16) -- 1e-14 leaves a factor of 12 and lies
# four (delta off by 1e-6 at d = 16) to thirteen orders below what the negative controls below produce.
TOL = 1e-14


@pytest.mark.parametrize("d", DEGREES)
def test_coefficients_match_the_interpolant(lib, d):
    pc = _library_coeffs(lib, d)
    ref = _reference(d)
    err = _value_error(pc, ref)
    assert err <= TOL, (d, err)
    # negative controls: the same assertion rejects a changed interval end, 1.6 / d instead of 1.6 / d^2, and the degree d - 1 interpolant
    for wrong in (_reference(d, delta=min(0.5, 1.6 / d ** 2) * (1 + 1e-6)), _reference(d, delta=min(0.5, 1.6 / d)) if d > 1 else None,
                  _reference(d - 1) if d > 1 else [mp.mpf(1)]):
        if wrong is None:
            continue
        assert _value_error(pc, wrong) > TOL, d


@pytest.mark.parametrize("d", DEGREES)
def test_interpolates_at_the_nodes_and_stays_positive(lib, d):
    """p(x_k) = f(x_k) at the d + 1 Chebyshev nodes (relative to sum |c_j|), and min p > 0.6 on [-1, 1]: L = p(N) is SPD on N's spectrum."""
    pc = _library_coeffs(lib, d)
    with mp.workdps(50):
        c = [mp.mpf(float(v)) for v in pc]
        scale = sum(abs(v) for v in c)
        delta = min(mp.mpf("0.5"), mp.mpf("1.6") / d ** 2)
        res = max(abs(_horner(c, x) - _f(x)) for x in _nodes(d, delta)) / scale
        assert float(res) <= TOL, (d, float(res))
        # negative control: the nodes of a shifted interval are not interpolated
        shifted = max(abs(_horner(c, x) - _f(x)) for x in _nodes(d, delta * (1 + mp.mpf("1e-3")))) / scale
        assert float(shifted) > TOL, d
        pmin = min(_horner(c, x) for x in _grid())
    assert float(pmin) > 0.6, (d, float(pmin))


def test_degree_outside_range_is_an_error(lib):
    L = lib.load()
    pc = np.zeros(18)
    for d in (0, -1, 17):
        assert L.dkmc_xtb_poly_coeffs(d, pc.ctypes.data_as(C.POINTER(C.c_double))) != 0, d
        assert b"degree" in L.dkmc_last_error()
        L.dkmc_clear_error()
    assert not pc.any()
