"""Host reference of the current map (dkmc_set_current_map) shared by the tests of the feature: the definitions of include/devicekmc_hip.h
evaluated in numpy on the CSR that dkmc_get_last_X exports, with the bounds both sides must meet.  Not a test module.

Tolerance (derived, not measured).  Device and host add the same products x_ic (m_i - m_c) of the same bits, each rounded once, so they differ
by summation rounding (any order: at most (n - 1) u sum|terms| per side, u = 2^-53) and one product rounding per term at the most:
  thr_all, thr_tun          |gpu - host| <= 4 n_i u host                    (n_i = stored entries of the row)
  net_tun, info[1], info[2] |gpu - host| <= 4 n_max u sum|J| of the row     (cancellation: relative to the terms, 2 thr of that row)
  info[3], info[4]          sums of the per-row values over R rows: the rows' own bounds plus the summation of R non-negative terms on either
                            side, 4 (n_max + R) u host
"""
import math

import numpy as np

U = 2.0 ** -53


def site_dist(ax, ay, az, a, b, laty, latz, pbc):
    """site_dist of csrc/common.h on index arrays a, b"""
    if pbc:
        dx = ax[a] - ax[b]
        fy = (ay[a] - ay[b]) / laty; fy = fy - np.round(fy)
        fz = (az[a] - az[b]) / latz; fz = fz - np.round(fz)
        dy, dz = fy * laty, fz * latz
        return np.sqrt(dx * dx + dy * dy + dz * dz)
    dx, dy, dz = ax[b] - ax[a], ay[b] - ay[a], az[b] - az[a]
    return np.sqrt(dx * dx + dy * dy + dz * dz)


def atom_sites(site_element):
    """site of atom a (the compaction of update_power: every site that is no DEFECT / OXYGEN_DEFECT, in site order)"""
    el = np.asarray(site_element)
    return np.flatnonzero((el != 0) & (el != 1))


def reference(X, m, ax, ay, az, atom_site, N, nn_dist, lattice, pbc):
    """X = (rp, ci, data) of dkmc_get_last_X; m = atom_virtual_potentials read after the call; ax, ay, az = atom positions of the buffer.
    Returns a dict: the three site arrays, info[1 .. 4], the per-site bounds and what the profile check needs."""
    rp, ci, data = X
    n = len(rp) - 1
    cnt = np.diff(rp).astype(np.int64)
    rows = np.repeat(np.arange(n), cnt)
    ci = np.asarray(ci, dtype=np.int64)
    off = (rows != ci) & (rows >= 2)
    r, c, x = rows[off], ci[off], data[off]
    J = x * (m[r] - m[c])
    pairs = np.flatnonzero(c >= 2)
    tun = np.zeros(len(c), dtype=bool)
    tun[pairs] = site_dist(ax, ay, az, r[pairs] - 2, c[pairs] - 2, lattice[1], lattice[2], pbc) >= nn_dist      # a pair of atom rows that is no neighbour pair: in T
    absJ = np.abs(J)
    row_abs = np.bincount(r, absJ, minlength=n)
    row_net = np.bincount(r, J, minlength=n)
    tun_abs = np.bincount(r[tun], absJ[tun], minlength=n)
    tun_net = np.bincount(r[tun], J[tun], minlength=n)
    n_max = int(cnt.max())
    site = np.asarray(atom_site)[np.arange(2, n) - 2]
    out = dict(n=n, n_max=n_max, site=site, has_row=np.zeros(N, dtype=bool))
    out["has_row"][site] = True
    for name, v in (("thr_all", 0.5 * row_abs), ("thr_tun", 0.5 * tun_abs), ("net_tun", tun_net)):
        a = np.zeros(N); a[site] = v[2:]; out[name] = a
    b = np.zeros(N); b[site] = 4.0 * cnt[2:] * U * 0.5 * row_abs[2:]; out["bound_thr_all"] = b
    b = np.zeros(N); b[site] = 4.0 * cnt[2:] * U * 0.5 * tun_abs[2:]; out["bound_thr_tun"] = b
    b = np.zeros(N); b[site] = 4.0 * n_max * U * tun_abs[2:]; out["bound_net_tun"] = b
    # info[1]: k_imacro's rule on row 0
    p0, p1 = int(rp[0]), int(rp[1])
    c0, x0 = ci[p0:p1], data[p0:p1]
    t0 = (x0 * (m[c0] - m[0]))[c0 >= 2]
    R = n - 2
    out["info"] = {1: float(t0.sum()), 2: float(np.abs(row_net[2:]).max()), 3: float(0.5 * row_abs[2:].sum()), 4: float(0.5 * tun_abs[2:].sum())}
    out["info_bound"] = {1: 4.0 * n_max * U * float(np.abs(t0).sum()), 2: 4.0 * n_max * U * float(row_abs[2:].max()),
                         3: 4.0 * (n_max + R) * U * float(0.5 * row_abs[2:].sum()), 4: 4.0 * (n_max + R) * U * float(0.5 * tun_abs[2:].sum())}
    out["tun_entries"] = (r[tun], c[tun], J[tun])
    return out


def check(got, info, ref, imacro=None):
    """got = (thr_all, thr_tun, net_tun) of the device, info = its eight doubles: every assertion of the feature's numerical contract"""
    for k, name in enumerate(("thr_all", "thr_tun", "net_tun")):
        g, h, b = got[k], ref[name], ref["bound_" + name]
        assert np.all(g[~ref["has_row"]] == 0.0), name                       # sites without a row: exactly zero
        bad = np.abs(g - h) > b
        assert not bad.any(), (name, int(bad.sum()), float(np.abs(g - h)[bad].max()), float(b[bad].min()))
    assert np.all(got[0] >= got[1]) and np.all(got[1] >= 0.0)
    for k in (1, 2, 3, 4):
        assert abs(info[k] - ref["info"][k]) <= ref["info_bound"][k], (k, info[k], ref["info"][k], ref["info_bound"][k])
    if imacro is not None:
        assert np.float64(info[0]).tobytes() == np.float64(imacro).tobytes()
    assert info[5] == ref["n"] - 2 and info[7] == 0.0
    # T is symmetric and every product is rounded once, the same bits at both ends: the exact sum of the device's values is its summation
    # rounding alone (a wrong sign on the column side would leave twice the net tunnelling current of the rows instead)
    assert abs(math.fsum(got[2])) <= float(ref["bound_net_tun"].sum())


def profile_reference(ref, site_x, cuts):
    """tunnelling current crossing x = cut: the classified entries with the row's site at or below the cut and the column's beyond it, and the
    bound of the per-row values summed over the rows of A"""
    r, c, J = ref["tun_entries"]
    site_x = np.asarray(site_x)
    xs = np.full(ref["n"], np.inf); xs[2:] = site_x[ref["site"]]
    out = []
    for cut in cuts:
        cross = (xs[r] <= cut) & ~(xs[c] <= cut)
        out.append((float(J[cross].sum()), float(ref["bound_net_tun"][site_x <= cut].sum())))
    return out
