"""Host reference of what update_power and the global temperature update make of a solved current system: the dissipated power per site
(k_power<64> on the CSR form; k_xt_gather_S + the rectified tile pass + k_xt_rows<1> + k_xt_power_rows on the tiled form), I_macro (k_imacro),
the shift of the node potentials (k_min_m, k_shift) and the two closed forms of the global temperature (k_power_partials, k_temp_update).  The
definitions are evaluated in numpy / math.fsum / decimal on data the tests read back: the CSR that dkmc_get_last_X exports, the potentials left
in atom_virtual_potentials and site_power.  Not a test module.  u = 2^-53 throughout.

Tolerances (derived, not measured).

site_power_reference.  Row i >= 2, stored column c >= 2, c != i:  d = m_i - m_c,  ical = fl(x_ic d),  term = fl(ical d);  the entry heats row i
iff (ical < 0 and Vd > 0) or (ical > 0 and Vd < 0);  power[site of i] = -alpha sum of the heating terms, non-metal atoms only.
  * every off-diagonal of X is <= 0, so every term x d^2 of a row has one sign: sum|terms| = |sum terms|, nothing cancels;
  * both sides form d = fl(m_i - m_c) from the same bits (the tiles see the pair from its row end only, d' = -d, and (x d')d' = (x d)d bit for
    bit), then the product with at most two roundings (one where the compiler contracts the second product into the sum): either side is within
    2 u |term| of x d d, so the two differ by 4 u |term| per term at the most;
  * summation in any order -- lanes, tiles, strips, records -- costs at most (n - 1) u sum|terms| per side over n terms, and a row of n_i stored
    entries has at most n_i - 1 terms (the diagonal is none); the host sums with fsum, which costs one rounding;
  * the predicate is the sign of ical, a single rounded product of identical operands: the same bit on both sides; where ical = 0 the term is 0
    whichever end takes it;
  * alpha multiplies once on each side (alpha = 1: exact).
  Together  |gpu - host| <= (4 + (n_i - 2) + 1 + 2) u sum|terms| <= 4 n_i u sum|terms|  for every n_i >= 2 (an atom row stores its diagonal and at
  least one neighbour).  The bound is  4 n_i u sum|heating terms|  of the row.

imacro_reference.  k_imacro's rule on row 1: the stored entries from rp[1] + 2 on (the kernel skips the first two by position: they must be the
columns 0 and 1, asserted here), columns >= 2, sum of x (m_c - m_1).  Same counting as above with one product per term: 4 n_1 u sum|terms|.

shift_reference.  m[0 : Na + 2] + |min(m[2 : Na + 2])|: the minimum is exact in any order and every element takes one addition of the same two
operands: bit for bit.

temperature_reference.  Both closed forms of k_temp_update from the same fp64 inputs, in decimal at 60 digits (Decimal(float) is exact).
  mode 0:  a = diss / C,  c = a T0 + P / C,  T = c/a + (T0 - c/a) exp(-a t);   T_steady = c/a = T0 + P/diss
    fp64 chain: a (1 rounding), a T0 (1), 1/C (1), (1/C) P (1), their sum (1), c/a (1): in s = c/a the error of a cancels between c's first term
    and the divisor, which leaves 3 u T0 + 5 u P/diss <= 5 u T_steady.  E = exp(-a t): 2 u on the argument (a, a t), worth 2 u (a t) E <= 0.74 u,
    plus 4 ulp for the call: 4.74 u E.  T = s (1 - E) + T0 E takes 5 u T_steady from s, 4.74 u |T0 - s| from E, one rounding each for T0 - s, the
    product and the last sum: (5 + 4.74 + 1 + 1 + 1) u T_steady < 13 u T_steady.
  mode 1:  cc = b + (P / C_thermal) small_step,  s = int(number_steps),  T = cc (1 - A^s)/(1 - A) + A^s T0;   T_steady = cc / (1 - A)
    fp64 chain: cc (3 roundings, all terms >= 0: 3 u cc), 1 - A (exact: A in [1/2, 1]), w = pow(A, s) (4 ulp), 1 - w (4 u w + 1 u), the product and
    the quotient (1 each): the first term is within (3 + 1 + 1 + 1 + 4) u T_steady, w T0 within (4 + 1) u T0, and the last sum adds 1 u of the larger:
    11 u T_steady + 6 u T0.
  Both are below the bound used:  16 u (|T_steady| + |T0|).  A contraction into fma removes roundings, never adds one.

power_sum_bound.  n non-negative terms summed in any order: (n - 1) u sum per side against the exact sum; n u fsum(p) is used.
"""
import math
from decimal import Decimal, localcontext

import numpy as np

U = 2.0 ** -53


def heating_entries(X, m, Vd):
    """The entries the power formula looks at, in stored order: rows r >= 2, columns c >= 2, c != r.  Returns a dict with r, c, x, the rounded
    products ical and term, heat (the entry heats its row end) and cnt (stored entries per row, the n_i of the bound)."""
    rp, ci, data = X
    n = len(rp) - 1
    cnt = np.diff(rp).astype(np.int64)
    rows = np.repeat(np.arange(n), cnt)
    ci = np.asarray(ci, dtype=np.int64)
    keep = (rows >= 2) & (ci >= 2) & (ci != rows)
    r, c, x = rows[keep], ci[keep], np.asarray(data, dtype=np.float64)[keep]
    m = np.asarray(m, dtype=np.float64)
    d = m[r] - m[c]
    ical = x * d
    term = ical * d
    heat = (ical < 0) if Vd > 0 else (ical > 0) if Vd < 0 else np.zeros(len(r), dtype=bool)
    return dict(n=n, cnt=cnt, r=r, c=c, x=x, ical=ical, term=term, heat=heat)


def row_sums(e, heat=None, keep=None):
    """per row of the system: fsum of the heating terms, sum of their magnitudes, their number.  heat / keep override the predicate or drop
    entries (the seeded faults of test_power_ref.py go through here)."""
    heat = e["heat"] if heat is None else heat
    if keep is not None:
        heat = heat & keep
    r, t = e["r"][heat], e["term"][heat]                               # (stored order: r ascending)
    n = e["n"]
    num = np.bincount(r, minlength=n)
    mag = np.bincount(r, np.abs(t), minlength=n)
    end = np.cumsum(num)
    val = np.zeros(n)
    for i in np.flatnonzero(num):
        val[i] = math.fsum(t[end[i] - num[i]:end[i]])
    return val, mag, num


def site_power_reference(X, m, Vd, atom_site, metal_atom, N, alpha=1.0, entries=None, heat=None, keep=None, rows=None):
    """X = (rp, ci, data) of dkmc_get_last_X; m = atom_virtual_potentials read after the call (scaled and shifted); atom_site[a] = site of atom
    a; metal_atom[a] = atom a is a contact metal.  Returns (power, written, bound), each of N sites: the values, the sites the row kernels write
    (the non-metal atoms that have a row: the system has Nsub - 2 = N_atom - 1 atom rows, the last atom has none) and 4 n_i u sum|terms|.
    entries / heat / keep / rows (atom rows evaluated, default all of them) let a caller evaluate a variant of the definition."""
    e = heating_entries(X, m, Vd) if entries is None else entries
    val, mag, _ = row_sums(e, heat, keep)
    n = e["n"]
    i = np.arange(2, n) if rows is None else np.asarray(rows)
    a = i - 2
    i, a = i[~np.asarray(metal_atom, dtype=bool)[a]], a[~np.asarray(metal_atom, dtype=bool)[a]]
    site = np.asarray(atom_site)[a]
    power, written, bound = np.zeros(N), np.zeros(N, dtype=bool), np.zeros(N)
    power[site] = -alpha * val[i]
    written[site] = True
    bound[site] = 4.0 * e["cnt"][i] * U * mag[i] * abs(alpha)
    return power, written, bound


def imacro_reference(X, m):
    """k_imacro's rule on row 1.  Returns (I_macro, bound, terms)."""
    rp, ci, data = X
    p0, p1 = int(rp[1]), int(rp[2])
    assert p1 - p0 >= 2 and int(ci[p0]) == 0 and int(ci[p0 + 1]) == 1          # the kernel skips the first two stored entries by position
    c = np.asarray(ci[p0 + 2:p1], dtype=np.int64)
    x = np.asarray(data[p0 + 2:p1], dtype=np.float64)
    m = np.asarray(m, dtype=np.float64)
    t = (x * (m[c] - m[1]))[c >= 2]
    return math.fsum(t), 4.0 * (p1 - p0) * U * math.fsum(np.abs(t)), t


def shift_reference(m_unshifted, Na):
    m = np.asarray(m_unshifted, dtype=np.float64)
    return m[0:Na + 2] + abs(m[2:Na + 2].min())


def temperature_reference(mode, P, T0, event_time=None, dissipation_constant=None, C=None,
                          a_coeff=None, b_coeff=None, number_steps=None, C_thermal=None, small_step=None):
    """mode 0: k_temp_update's a0, a1, a2 = event_time, dissipation_constant, C (= A t_ox c_p 1e6, formed in fp64 by the caller as the library
    does); mode 1: a_coeff, b_coeff, number_steps, C_thermal, small_step.  Returns (T, bound, T_steady) as floats."""
    with localcontext() as ctx:
        ctx.prec = 60
        D = Decimal
        P, T0 = D(float(P)), D(float(T0))
        if mode == 0:
            a = D(float(dissipation_constant)) / D(float(C))
            c = a * T0 + P / D(float(C))
            steady = c / a
            T = steady + (T0 - steady) * (-a * D(float(event_time))).exp()
        else:
            A = D(float(a_coeff))
            cc = D(float(b_coeff)) + P / D(float(C_thermal)) * D(float(small_step))
            s = int(number_steps)
            assert 0 <= s < 2 ** 31 and A > 0
            w = (D(s) * A.ln()).exp() if s else D(1)
            steady = cc / (1 - A)
            T = cc * (1 - w) / (1 - A) + w * T0
        bound = 16.0 * U * (abs(float(steady)) + abs(float(T0)))
        return float(T), bound, float(steady)


def temperature_fp64(mode, P, T0, event_time=None, dissipation_constant=None, C=None,
                     a_coeff=None, b_coeff=None, number_steps=None, C_thermal=None, small_step=None):
    """the statements of k_temp_update in plain fp64 Python (what the bound is validated on without a GPU)"""
    if mode == 0:
        a = dissipation_constant / C
        c = (dissipation_constant / C) * T0 + (1 / C) * P
        return (c / a) + (T0 - c / a) * math.exp(-a * event_time)
    c_coeff = b_coeff + P / C_thermal * small_step
    step = int(number_steps)
    return c_coeff * (1.0 - math.pow(a_coeff, float(step))) / (1.0 - a_coeff) + math.pow(a_coeff, float(step)) * T0


def power_sum_bound(p):
    """non-negative terms summed in any order: |sum - fsum(p)| <= len(p) u fsum(p)"""
    p = np.asarray(p, dtype=np.float64)
    assert np.all(p >= 0)
    return len(p) * U * math.fsum(p)
