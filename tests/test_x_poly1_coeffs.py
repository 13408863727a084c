"""Coefficients of the one-polynomial form of the preconditioner (dkmc_set_x_poly_form; csrc/xtb_precond.h: xtb_poly1_coeffs, through dkmc_xtb_poly1_coeffs):
q is the Chebyshev interpolant of degree n of (1 - x)^-1 on [-1, 1 - min(0.5, 3.2 / n^2)] in the monomial basis.  q(N) stands for M^-1 in the loop, so it
has to be positive on the whole of [-1, 1], and its smallest value there scales the loop's stop test.  Host code only, no GPU needed."""
import ctypes as C

import numpy as np
import pytest
from numpy.polynomial import Polynomial, chebyshev

DEGREES = [1, 8, 10, 16, 20]
DP = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from devicekmc_amd import lib as L
    return L


def _library(lib, n):
    pc = np.full(22, np.nan)
    qmin = C.c_double(np.nan)
    lib.check(lib.load().dkmc_xtb_poly1_coeffs(n, pc.ctypes.data_as(DP), C.byref(qmin)))
    assert np.all(np.isfinite(pc[:n + 1])) and np.all(np.isnan(pc[n + 1:])), pc          # exactly n + 1 coefficients written
    return pc[:n + 1], qmin.value


def _numpy_interpolant(n):
    """the same interpolant by numpy: Chebyshev coefficients of f(x(t)) on t in [-1, 1], then powers of t, then t = al x + be"""
    a, b = -1.0, 1.0 - min(0.5, 3.2 / n ** 2)
    c = chebyshev.chebinterpolate(lambda t: 1.0 / (1.0 - (0.5 * (b - a) * t + 0.5 * (b + a))), n)
    pt = Polynomial(chebyshev.cheb2poly(c))
    px = pt(Polynomial([-(a + b) / (b - a), 2.0 / (b - a)]))
    out = np.zeros(n + 1)
    out[:len(px.coef)] = px.coef
    return out


def _sample(pc):
    x = -1.0 + np.arange(4001) / 2000.0
    q = np.full_like(x, pc[-1])
    for cj in pc[-2::-1]:
        q = q * x + cj
    return x, q


@pytest.mark.parametrize("n", DEGREES)
def test_coefficients_equal_the_numpy_interpolant(lib, n):
    pc, _ = _library(lib, n)
    want = _numpy_interpolant(n)
    err = np.abs(pc - want).max() / np.abs(want).max()
    print("n = %d: max |c - numpy| / max |c| = %.2e, max |c| = %.3e" % (n, err, np.abs(want).max()))
    assert err <= 1e-12, (n, err)
    # negative control: the interpolant of (1 - x)^(-1/2), and the one on the split form's interval, are other polynomials
    a, b = -1.0, 1.0 - min(0.5, 1.6 / n ** 2)
    other = chebyshev.chebinterpolate(lambda t: 1.0 / (1.0 - (0.5 * (b - a) * t + 0.5 * (b + a))), n)
    px = Polynomial(chebyshev.cheb2poly(other))(Polynomial([-(a + b) / (b - a), 2.0 / (b - a)])).coef
    if n > 1:                                                               # (n = 1: both intervals end at 0.5)
        assert np.abs(pc - px).max() / np.abs(want).max() > 1e-12, n


@pytest.mark.parametrize("n", DEGREES)
def test_positive_on_the_interval_and_the_minimum_is_the_sampled_one(lib, n):
    pc, qmin = _library(lib, n)
    x, q = _sample(pc)
    print("n = %d: min q on [-1, 1] = %.6f at x = %.4f (library: %.6f)" % (n, q.min(), x[q.argmin()], qmin))
    assert q.min() > 0.0, (n, q.min())
    assert abs(qmin - q.min()) <= 1e-12 * np.abs(pc).max(), (n, qmin, q.min())      # the same Horner sums up to their rounding (max |c| is their scale)


def test_degree_outside_range_is_an_error(lib):
    L = lib.load()
    pc = np.zeros(24)
    for n in (0, 21, -1):
        assert L.dkmc_xtb_poly1_coeffs(n, pc.ctypes.data_as(DP), None) != 0, n
        assert b"degree" in L.dkmc_last_error()
        L.dkmc_clear_error()
    assert not pc.any()


def test_declared_in_the_debug_header_and_the_ctypes_table():
    import os
    from devicekmc_amd import lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dbg = open(os.path.join(root, "include", "devicekmc_hip_debug.h")).read()
    pub = open(os.path.join(root, "include", "devicekmc_hip.h")).read()
    for name, src in (("dkmc_xtb_poly1_coeffs", dbg), ("dkmc_xtb_test_gram1", dbg), ("dkmc_xtb_test_step1", dbg), ("dkmc_debug_set_x_poly1_degree", dbg),
                      ("dkmc_set_x_poly_form", pub), ("dkmc_get_x_poly_form", pub), ("dkmc_get_x_poly_form_used", pub), ("dkmc_get_x_poly_products", pub)):
        assert name + "(" in src and name in L.SYMBOLS, name
