"""Extended-precision restatement of the screened pair sum (dkmc_poisson_gridless_gpu, csrc/potential.hip from k_charge_flags on) and the synthetic
boxes its tests run on.  No GPU and no oracle in here: tests/test_pair_sum_ref.py pins pair_sum_ref to the oracle and to a 40-digit evaluation and
checks every case's inputs; tests/test_gpu_pair_sum_boxes.py compares the kernels with it.

pair_sum_ref: per site the sum over all charged sites j != i of q_j erfc(r / (sigma sqrt 2)) k Q / r (v_solve, csrc/common.h), r in metres -- over
every pair (v_all) and over the pairs with d2 <= cut2 only (v_in), with the sum of magnitudes (abs_in) and the number (n_in) of the latter.  d2
follows pw_d2 (with pbc the fractional difference along y and z minus its round(); x is never periodic) in np.longdouble from the float64
coordinates; erfc is scipy's on the float64-rounded argument (corrected to first order for that rounding, which a 40-digit evaluation sees on
sites whose every charged neighbour is far away); every sum is accumulated in np.longdouble.  A pair is excluded by site index, never
by distance.  margin = min over all pairs of |d2 / cut2 - 1|: how far the inputs keep every pair from the cut-off.

pair_grid_ref: the column grid k_pw_grid decides on, so that every case can state which branch of the kernels it reaches.

CASES: name -> generator (fixed seed) of a Case.  A Case carries one point set and a list of `steps`, each a charge vector with the grid it must
give; all cases but `threshold` have one step."""
import functools
import math
from typing import List, NamedTuple, Tuple

import numpy as np

from devicekmc_amd import params as _params

LD = np.longdouble
Q = _params.KMCParameters().q                  # DKMC_Q of csrc/common.h
K = _params.KMCParameters().k
XCUT = 6.5                                     # PW_CUT
PW_MAXDIM, PW_MAXX, PW_MIN_CHARGED, PW_SITES, PW_SORTCAP = 32, 16, 512, 64, 8192


class PairRef(NamedTuple):
    v_all: np.ndarray          # longdouble [N]
    v_in: np.ndarray           # longdouble [N]
    abs_in: np.ndarray         # longdouble [N]
    n_in: np.ndarray           # int64 [N]
    margin: float              # min |d2 / cut2 - 1| over all pairs
    d2_min: float              # smallest d2 [A^2] between a site and a charged site other than itself


def cut2_of(sigma, xcut):
    """cut2 [A^2] as the kernels form it (float64); 0 switches the cut-off off."""
    rc = xcut * sigma * math.sqrt(2.0) * 1e10
    return rc * rc if xcut > 0.0 else math.inf


def _round_half_away(f):
    return np.sign(f) * np.floor(np.abs(f) + LD(0.5))          # C round()


def pair_d2(xi, yi, zi, xj, yj, zj, lattice, pbc):
    """pw_d2 in np.longdouble; the arguments broadcast."""
    xi, yi, zi, xj, yj, zj = (np.asarray(a, dtype=np.float64).astype(LD) for a in (xi, yi, zi, xj, yj, zj))
    dx = xi - xj
    if pbc:
        ly, lz = LD(lattice[1]), LD(lattice[2])
        fy = (yi - yj) / ly; fy = fy - _round_half_away(fy)
        fz = (zi - zj) / lz; fz = fz - _round_half_away(fz)
        dy, dz = fy * ly, fz * lz
    else:
        dy, dz = yi - yj, zi - zj
    return dx * dx + dy * dy + dz * dz


def _pair_d2_f64(xi, yi, zi, xj, yj, zj, lattice, pbc):
    dx = xi - xj
    if pbc:
        fy = (yi - yj) / lattice[1]; fy = fy - np.sign(fy) * np.floor(np.abs(fy) + 0.5)
        fz = (zi - zj) / lattice[2]; fz = fz - np.sign(fz) * np.floor(np.abs(fz) + 0.5)
        dy, dz = fy * lattice[1], fz * lattice[2]
    else:
        dy, dz = yi - yj, zi - zj
    return dx * dx + dy * dy + dz * dz


A_ZERO = 28.0          # erfc(a) and exp(-a^2) are exactly 0.0 in float64 from a = 27.3 on: such a pair adds exactly nothing to any sum below


def pair_sum_ref(x, y, z, lattice, pbc, sigma, k, q, xcut, chunk_pairs=1 << 21):
    """The sums in row chunks of at most chunk_pairs pairs.  A float64 pass over a chunk picks the pairs with r / (sigma sqrt 2) <= A_ZERO (all of them
    when the cut-off is off); only those go through np.longdouble -- the others' terms are exact zeros and they lie 17 cut-offs out."""
    from scipy.special import erfc
    x, y, z = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, y, z))
    q = np.asarray(q)
    N = len(x)
    cj = np.flatnonzero(q)
    nq = len(cj)
    v_all, v_in, abs_in = np.zeros(N, dtype=LD), np.zeros(N, dtype=LD), np.zeros(N, dtype=LD)
    n_in = np.zeros(N, dtype=np.int64)
    margin, d2_min = math.inf, math.inf
    if nq == 0:
        return PairRef(v_all, v_in, abs_in, n_in, margin, d2_min)
    cut2 = LD(cut2_of(float(sigma), float(xcut)))
    finite = bool(np.isfinite(float(cut2)))
    zero2 = (A_ZERO * float(sigma) * math.sqrt(2.0) * 1e10) ** 2 if finite else math.inf
    assert zero2 > 4.0 * float(cut2) or not finite
    qc = q[cj].astype(LD)
    kq = LD(float(k)) * LD(Q)
    s2 = LD(float(sigma)) * np.sqrt(LD(2))
    two_over_sqrt_pi = LD(2) / np.sqrt(np.arctan(LD(1)) * LD(4))
    rows = max(1, chunk_pairs // nq)

    def row_sums(v, start, empty):
        out = np.add.reduceat(np.concatenate([v, np.zeros(1, dtype=v.dtype)]), start)      # (the sentinel keeps every start a valid index)
        out[empty] = 0
        return out

    for r0 in range(0, N, rows):
        r1 = min(N, r0 + rows)
        d64 = _pair_d2_f64(x[r0:r1, None], y[r0:r1, None], z[r0:r1, None], x[None, cj], y[None, cj], z[None, cj], lattice, pbc)
        own = np.arange(r0, r1)[:, None] == cj[None, :]                # a pair is excluded by site index
        near = ~own & (d64 <= zero2)
        far = ~own & ~near
        if far.any():
            d2_min = min(d2_min, float(d64[far].min()))
            margin = min(margin, float(np.abs(d64[far] / float(cut2) - 1.0).min()))      # (>= 17: it never decides the minimum of a case with any pair in reach)
        ri, ci = np.nonzero(near)                                      # row-major: ri ascending
        if len(ri) == 0:
            continue
        gi, gj = r0 + ri, cj[ci]
        d2 = pair_d2(x[gi], y[gi], z[gi], x[gj], y[gj], z[gj], lattice, pbc)
        r = LD(1e-10) * np.sqrt(d2)
        a = r / s2
        a64 = a.astype(np.float64)                 # scipy's erfc there, plus the first-order term of what the rounding of the argument left out:
        e = erfc(a64).astype(LD) - two_over_sqrt_pi * np.exp(-a64 * a64).astype(LD) * (a - a64)      # erfc' = -2 / sqrt(pi) exp(-a^2); at a = 10 it is worth 200 ulp
        term = qc[ci] * e * kq / r
        inside = d2 <= cut2
        tin = np.where(inside, term, LD(0))
        start = np.searchsorted(ri, np.arange(r1 - r0))
        empty = np.bincount(ri, minlength=r1 - r0) == 0
        v_all[r0:r1] = row_sums(term, start, empty)
        v_in[r0:r1] = row_sums(tin, start, empty)
        abs_in[r0:r1] = row_sums(np.abs(tin), start, empty)
        n_in[r0:r1] = np.bincount(ri[inside], minlength=r1 - r0)
        d2_min = min(d2_min, float(d2.min()))
        if finite:
            margin = min(margin, float(np.abs(d2 / cut2 - LD(1)).min()))
    return PairRef(v_all, v_in, abs_in, n_in, margin, d2_min)


def pair_grid_ref(lattice, sigma, xcut, ncharged):
    """(ny, nz, ry, rz, nx, use) by the rule of k_pw_grid."""
    if not xcut > 0.0:
        return 1, 1, 0, 0, 1, 0
    rc = xcut * sigma * math.sqrt(2.0) * 1e10
    ny = max(1, min(PW_MAXDIM, int(math.floor(2.0 * lattice[1] / rc))))
    nz = max(1, min(PW_MAXDIM, int(math.floor(2.0 * lattice[2] / rc))))
    ry, rz = int(math.ceil(rc / (lattice[1] / ny))), int(math.ceil(rc / (lattice[2] / nz)))
    nx = max(1, min(PW_MAXX, int(math.floor(4.0 * lattice[0] / rc))))
    use = (ny >= 2 * ry + 1 or nz >= 2 * rz + 1) and min(2 * ry + 1, ny) * min(2 * rz + 1, nz) <= 32 and ncharged >= PW_MIN_CHARGED
    return ny, nz, ry, rz, nx, int(use)


def column_of(y, z, lattice, ny, nz, pbc):
    """Column index of k_pw_bin (pw_axis_cell), float64 as on the device."""
    def axis(v, L, n):
        v = np.asarray(v, dtype=np.float64)
        if pbc:
            f = v / L; f = f - np.floor(f)
            return np.minimum((f * n).astype(np.int64), n - 1)
        return np.clip(np.floor(v / (L / n)).astype(np.int64), 0, n - 1)
    return axis(z, lattice[2], nz) * ny + axis(y, lattice[1], ny)


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------
class Step(NamedTuple):
    q: np.ndarray                               # int32 [N]
    grid: Tuple[int, int, int, int, int, int]   # (ny, nz, ry, rz, nx, use) this step must give


class Case(NamedTuple):
    name: str
    lattice: Tuple[float, float, float]
    sigma: float
    x: np.ndarray
    y: np.ndarray
    z: np.ndarray
    steps: List[Step]
    pbcs: Tuple[int, ...]                       # the pbc values the case runs with
    probes: np.ndarray                          # 8 sites for the 40-digit check: first, last, 6 drawn
    tested_below: float = 0.0                   # > 0: the cell list must distance-test fewer than this fraction of N nq pairs
    same_as: str = ""                           # a case whose potentials this one must reproduce site by site

    @property
    def N(self):
        return len(self.x)


def _charges(rng, N, nq, allowed=None):
    q = np.zeros(N, dtype=np.int32)
    pool = np.arange(N) if allowed is None else np.flatnonzero(allowed)
    q[rng.choice(pool, nq, replace=False)] = rng.choice(np.array([-2, -1, 1, 2], dtype=np.int32), nq)
    return q


def _probes(rng, N):
    return np.concatenate([[0, N - 1], rng.choice(np.arange(1, N - 1), 6, replace=False)]).astype(np.int64)


def _uniform(name, seed, lattice, N, nq, grid, sigma=1e-10, pbcs=(0,), **kw):
    rng = np.random.default_rng(seed)
    x, y, z = (rng.random(N) * L for L in lattice)
    q = _charges(rng, N, nq)
    return Case(name, tuple(lattice), sigma, x, y, z, [Step(q, grid)], pbcs, _probes(rng, N), **kw)


BOTH_PBC = ("rect", "rect_T", "narrow_z", "outside")      # the cases that also run periodic in y and z; the others run open only
RECT_BOX = (30.0, 60.0, 25.0)
RECT_GRID = (13, 5, 2, 2, 13, 1)


@functools.lru_cache(maxsize=None)
def _rect():
    return _uniform("rect", 101, RECT_BOX, 6000, 800, RECT_GRID, pbcs=(0, 1))


@functools.lru_cache(maxsize=None)
def _rect_T():
    c = _rect()
    lx, ly, lz = c.lattice
    return c._replace(name="rect_T", lattice=(lx, lz, ly), y=c.z, z=c.y, steps=[Step(c.steps[0].q, (5, 13, 2, 2, 13, 1))], same_as="rect")


@functools.lru_cache(maxsize=None)
def _holes():
    """A checkerboard of the 13 x 5 columns: columns 0 (first) and 64 (last) and every second interior one are empty.  One occupied column holds
    exactly 64 sites, one 65; no charged site in a quarter of the occupied columns.  Site order shuffled."""
    rng = np.random.default_rng(108)
    lx, ly, lz = RECT_BOX
    ny, nz = 13, 5
    occ = np.array([c for c in range(ny * nz) if (c % ny + c // ny) % 2 == 1])
    N, nq = 6000, 800
    col = np.concatenate([np.full(64, occ[5]), np.full(65, occ[20]), rng.choice(np.delete(occ, [5, 20]), N - 129)])
    col = col[rng.permutation(N)]
    x = rng.random(N) * lx
    y = (col % ny + 0.02 + 0.96 * rng.random(N)) * (ly / ny)
    z = (col // ny + 0.02 + 0.96 * rng.random(N)) * (lz / nz)
    bare = rng.choice(occ, len(occ) // 4, replace=False)
    q = _charges(rng, N, nq, allowed=~np.isin(col, bare))
    return Case("holes", RECT_BOX, 1e-10, x, y, z, [Step(q, RECT_GRID)], (0,), _probes(rng, N))


@functools.lru_cache(maxsize=None)
def _outside():
    """rect's box; 5 % of the sites up to 1.5 box lengths outside it in y or z, 5 % at x < 0 or x > lx, 20 sites exactly on y = 0, y = ly and
    multiples of ly / ny."""
    rng = np.random.default_rng(109)
    lx, ly, lz = RECT_BOX
    N, nq = 6000, 800
    x, y, z = rng.random(N) * lx, rng.random(N) * ly, rng.random(N) * lz
    who = rng.permutation(N)
    lat_out, x_out, face = who[:300], who[300:600], who[600:620]
    for n, i in enumerate(lat_out):
        L, v = (ly, y) if n % 2 == 0 else (lz, z)
        d = 1.5 * L * rng.random()
        v[i] = -d if (n // 2) % 2 == 0 else L + d
    for n, i in enumerate(x_out):
        d = 15.0 * rng.random()
        x[i] = -d if n % 2 == 0 else lx + d
    y[face] = np.array([0.0, ly, 0.0, ly] + [m * (ly / 13) for m in range(1, 13)] + [m * (ly / 13) for m in (3, 6, 9, 12)])
    q = _charges(rng, N, nq)
    return Case("outside", RECT_BOX, 1e-10, x, y, z, [Step(q, RECT_GRID)], (0, 1), _probes(rng, N))


@functools.lru_cache(maxsize=None)
def _long_x():
    rng = np.random.default_rng(111)
    lat = (150.0, 60.0, 25.0)
    N, nq = 8000, 800
    u = rng.random(N) * 10.0
    x = np.where(rng.random(N) < 0.5, u, 150.0 - u)
    y, z = rng.random(N) * lat[1], rng.random(N) * lat[2]
    q = _charges(rng, N, nq)
    return Case("long_x", lat, 1e-10, x, y, z, [Step(q, (13, 5, 2, 2, 16, 1))], (0,), _probes(rng, N), tested_below=0.6)


@functools.lru_cache(maxsize=None)
def _big_segment():
    """9 000 of the 12 000 sites inside column (6, 2) of the 13 x 5 grid; nx = 1, so its one (column, bin) segment exceeds PW_SORTCAP."""
    rng = np.random.default_rng(112)
    lat = (2.0, 60.0, 25.0)
    N, nq, dense = 12000, 700, 9000
    x, y, z = rng.random(N) * lat[0], rng.random(N) * lat[1], rng.random(N) * lat[2]
    who = rng.permutation(N)[:dense]
    y[who] = (6 + 0.02 + 0.96 * rng.random(dense)) * (lat[1] / 13)
    z[who] = (2 + 0.02 + 0.96 * rng.random(dense)) * (lat[2] / 5)
    q = _charges(rng, N, nq)
    return Case("big_segment", lat, 1e-10, x, y, z, [Step(q, (13, 5, 2, 2, 1, 1))], (0,), _probes(rng, N))


@functools.lru_cache(maxsize=None)
def _threshold():
    """rect's points; exactly 512 charged (cell list), then 511 (k_pairwise), then 512 again -- on one cached grouping, no reset in between."""
    c = _rect()
    q512 = c.steps[0].q.copy()
    q512[np.flatnonzero(q512)[512:]] = 0
    q511 = q512.copy()
    q511[np.flatnonzero(q511)[-1]] = 0
    on, off = RECT_GRID, RECT_GRID[:5] + (0,)
    return c._replace(name="threshold", steps=[Step(q512, on), Step(q511, off), Step(q512, on)], pbcs=(0,))


CASES = {
    "rect": _rect,
    "rect_T": _rect_T,
    "narrow_z": lambda: _uniform("narrow_z", 103, (30.0, 60.0, 12.0), 5000, 700, (13, 2, 2, 2, 13, 1), pbcs=(0, 1)),
    "sliver_z": lambda: _uniform("sliver_z", 104, (30.0, 60.0, 4.0), 4000, 600, (13, 1, 2, 3, 13, 1)),
    "both_narrow": lambda: _uniform("both_narrow", 105, (30.0, 20.0, 20.0), 5000, 700, (4, 4, 2, 2, 13, 0)),
    "clamp_y": lambda: _uniform("clamp_y", 106, (20.0, 200.0, 25.0), 8000, 1000, (32, 5, 2, 2, 8, 1)),
    "full_grid": lambda: _uniform("full_grid", 107, (12.0, 320.0, 320.0), 20000, 2000, (32, 32, 1, 1, 5, 1)),
    "holes": _holes,
    "outside": _outside,
    "thin_x": lambda: _uniform("thin_x", 110, (2.0, 60.0, 25.0), 4000, 600, (13, 5, 2, 2, 1, 1)),
    "long_x": _long_x,
    "big_segment": _big_segment,
    "physical": lambda: _uniform("physical", 113, (40.0, 100.0, 170.0), 8000, 900, (6, 10, 2, 2, 4, 1), sigma=3.5e-10),
    "threshold": _threshold,
}
RUNS = [(name, pbc) for name in CASES for pbc in ((0, 1) if name in BOTH_PBC else (0,))]       # what a test parametrises over, without generating a case


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name, pbc, step=0):
    """pair_sum_ref of one step of a case at the default cut-off: computed once per process, shared, never written to."""
    c = case(name)
    if name == "threshold" and step == 2:
        return reference(name, pbc, 0)
    ref = pair_sum_ref(c.x, c.y, c.z, c.lattice, pbc, c.sigma, K, c.steps[step].q, XCUT)
    for a in ref[:4]:
        a.setflags(write=False)
    return ref
