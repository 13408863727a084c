#!/usr/bin/env python3
"""CPU experiment behind dkmc_set_x_stop_form: the one-polynomial block loop of csrc/xtb.hip in its own variables -- Pt, Pi = M Pt,
Q = A Pt, U = q(N) Q, Rt, Z = q(N) Rt kept by recurrence, the s x s algebra of k_xtb_small -- on the oracle's Jacobi-scaled X, from a zero start (step 1)
and from the previous step's solution (step 2, the warm regime).  Per sweep it records ||Rt+(:, 0)||_2 and (Rt+'Z+)_00 and reports the sweep at which
each stop rule fires first:

  bound      (Rt+'Z+)_00 <= tol^2 min q          the loop's test (k_xtb_small; tol2_loop of xtb_cg_body)
  norm k     ||Rt+(:, 0)||_2 <= k tol            the contract's quantity with a margin k in {1, 0.8, 1 / 1.5}

together with the TRUE residual ||A y - b|| of column 0 at that sweep.  q: the library's own coefficients (dkmc_xtb_poly1_coeffs; host code, no GPU).
usage: python tools/x_stop_norm_proto.py [2.5nm|7.5nm] [degree ...]          (default degrees: 10 18)"""
import ctypes
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import blockcg_proto as bp  # noqa: E402
from devicekmc_amd import lib  # noqa: E402
from oracle import oracle as oc  # noqa: E402

KAPPAS = (1.0, 0.8, 1.0 / 1.5)
TOL = 1e-6


def scaled(o, p, Vd):
    X = o.assemble_X()
    Na = X["Na"]; m = Na + 1
    A = sp.csr_matrix((X["data"], X["col"], X["row_ptr"][:m + 1]), shape=(m, Na + 2))[:, :m].tocsr()
    b = np.zeros(m); b[0] = -p.X_loop_G * Vd; b[1] = p.X_loop_G * Vd
    sc = 1.0 / np.sqrt(A.diagonal())
    return (sp.diags(sc) @ A @ sp.diags(sc)).tocsr(), b * sc, sc


def neighbour_N(o, As):
    """N = I - An, An = neighbour part + driver rows + unit diagonal of the scaled X (tools/precond_block_proto.py)"""
    m = As.shape[0]
    L_ = oc.lib()
    atom_site = np.empty(o.N, dtype=np.int32)
    Na = L_.okmc_compact_atoms(o.N, oc._p(o.element), oc._p(atom_site)); atom_site = atom_site[:Na].copy()
    an = np.empty((Na, o.nn), dtype=np.int32)
    L_.okmc_atom_neighbors(o.N, o.nn, oc._p(o.neigh), Na, oc._p(atom_site), oc._p(an))
    rows = np.repeat(np.arange(Na), o.nn); cols = an.ravel(); keep = cols >= 0
    Pn = sp.csr_matrix((np.ones(keep.sum()), (rows[keep] + 2, cols[keep] + 2)), shape=(Na + 2, Na + 2))[:m, :m]
    Pn = ((Pn + Pn.T) > 0).astype(np.float64).tolil()
    Pn[0:2, :] = 1.0; Pn[:, 0:2] = 1.0
    Pn.setdiag(1.0)
    N = (sp.identity(m, format="csr") - As.multiply(Pn.tocsr())).tocsr(); N.eliminate_zeros()
    return N


def poly1(n):
    pc = (ctypes.c_double * (n + 1))(); qmin = ctypes.c_double()
    rc = lib.load().dkmc_xtb_poly1_coeffs(n, pc, ctypes.byref(qmin))
    assert rc == 0
    return np.array(pc[:]), qmin.value


def qN(N, pc, V):
    out = pc[-1] * V
    for c in pc[-2::-1]:
        out = N @ out + c * V
    return out


def sym(G):
    return 0.5 * (G + G.T)


def loop(As, N, pc, qmin, b, y0, s=16, maxit=400, floor=0.3):
    """the one-polynomial block loop; runs until every rule has fired and the norm is `floor` below the tightest margin.  Returns the per-sweep records"""
    m = len(b)
    B = np.empty((m, s)); B[:, 0] = b; B[:, 1:] = bp.aux_rhs(m, s) * np.linalg.norm(b) / np.sqrt(m)
    Y = np.zeros((m, s)); Y[:, 0] = y0
    Rt = As @ Y - B
    Z = qN(N, pc, Rt)
    G = sym(Rt.T @ Z)
    W = np.linalg.inv(np.linalg.cholesky(G)).T
    Pt = -Z @ W; Pi = -Rt @ W
    rec = [dict(sweep=0, norm=float(np.linalg.norm(Rt[:, 0])), rz=float(G[0, 0]), true=float(np.linalg.norm(As @ Y[:, 0] - b)))]
    for it in range(1, maxit + 1):
        Q = As @ Pt
        U = qN(N, pc, Q)
        Gpt = sym(Pt.T @ Q); Gpr = Pt.T @ Rt; Gtr = Q.T @ Z; Gtt = sym(Q.T @ U); Grr = sym(Rt.T @ Z); Gpp = sym(Pt.T @ Pi)
        c = -np.linalg.solve(Gpt, Gpr)
        V = Gtt @ c + Gtr
        beta = np.linalg.solve(Gpt, V)
        Grn = sym(Grr + c.T @ V + Gtr.T @ c)
        Gprn = Gpt @ c + Gpr
        Gg = sym(beta.T @ (Gpp @ beta) + Grn - beta.T @ Gprn - Gprn.T @ beta)
        try:
            W = np.linalg.inv(np.linalg.cholesky(Gg)).T
        except np.linalg.LinAlgError:
            W = np.diag(1.0 / np.sqrt(np.diag(Gg)))
        Y = Y + Pt @ c
        Rn = Rt + Q @ c; Zn = Z + U @ c
        Pt, Pi = (-Zn + Pt @ beta) @ W, (-Rn + Pi @ beta) @ W
        Rt, Z = Rn, Zn
        rec.append(dict(sweep=it, norm=float(np.linalg.norm(Rt[:, 0])), rz=float(Grn[0, 0]), rz_direct=float(Rt[:, 0] @ Z[:, 0]),
                        true=float(np.linalg.norm(As @ Y[:, 0] - b))))
        if rec[-1]["norm"] <= floor * min(KAPPAS) * TOL and rec[-1]["rz"] <= TOL * TOL * qmin:
            break
    return rec, Y[:, 0]


def first(rec, pred):
    for r in rec[1:]:
        if pred(r):
            return r
    return None


def report(tag, n, qmin, rec):
    out = dict(case=tag, degree=n, qmin=qmin, tol=TOL, rules={})
    rb = first(rec, lambda r: not (r["rz"] > TOL * TOL * qmin))
    out["rules"]["bound"] = dict(sweep=rb["sweep"], norm=rb["norm"], true=rb["true"]) if rb else None
    for k in KAPPAS:
        rk = first(rec, lambda r: r["norm"] <= k * TOL)
        out["rules"]["norm %.3f" % k] = dict(sweep=rk["sweep"], norm=rk["norm"], true=rk["true"]) if rk else None
    ratio = [r["rz"] / (qmin * r["norm"] ** 2) for r in rec[1:] if r["norm"] > 0]
    out["rz_over_qmin_norm2"] = [min(ratio), max(ratio)]
    out["per_sweep"] = [[r["sweep"], float("%.4e" % r["norm"]), float("%.4e" % r["rz"]), float("%.4e" % r["true"])] for r in rec]
    return out


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "2.5nm"
    degrees = [int(x) for x in sys.argv[2:]] or [10, 18]
    Vd = 5.0
    s, p = bp.load(name)
    o = oc.OracleKMC(s.element, s.x, s.y, s.z, p)
    o.set_laplace_potential(Vd)
    systems = []
    t0 = time.time()
    for _ in range(2):
        o.update_charge(); o.update_potential(Vd); o.execute_kmc_step()
        As, b, sc = scaled(o, p, Vd)
        systems.append((As, b, sc, neighbour_N(o, As)))
    print("# %s: %d rows, %d nnz (two steps assembled in %.0f s)" % (name, len(systems[0][1]), systems[0][0].nnz, time.time() - t0), file=sys.stderr, flush=True)
    for n in degrees:
        pc, qmin = poly1(n)
        As, b, sc, N = systems[0]
        t0 = time.time()
        rec, y = loop(As, N, pc, qmin, b, np.zeros(len(b)))
        print(json.dumps(report("%s cold (zero start, step 1)" % name, n, qmin, rec)), flush=True)
        As2, b2, sc2, N2 = systems[1]
        rec2, _ = loop(As2, N2, pc, qmin, b2, y * sc / sc2)            # the unscaled solution of step 1, in step 2's scaling
        print(json.dumps(report("%s warm (step 2 from step 1's solution)" % name, n, qmin, rec2)), flush=True)
        print("# degree %d: %d + %d sweeps run [%.0f s]" % (n, len(rec) - 1, len(rec2) - 1, time.time() - t0), file=sys.stderr, flush=True)


if __name__ == "__main__":
    main()
