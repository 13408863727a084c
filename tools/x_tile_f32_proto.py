#!/usr/bin/env python3
"""CPU experiment behind dkmc_set_x_tile_f32: the block-CG of csrc/xtb.hip (width 16) on the split-preconditioned operator
L A L (degree 8, tools/precond_block_proto.py) at tol 1e-6, run twice on the oracle's X: with the tunnelling entries At = A - An as they are, and with
every stored (unscaled) tunnelling entry rounded to float32 INSIDE THE LOOP ONLY -- the right-hand side, L, the neighbour part, the diagonal, the Jacobi
scaling and the final true-residual check stay fp64, as on the device.  The loop stops on the recurrence residual of L A L at tol / 1.5 (xtb_cg_body).
Passes if the true fp64 residual of column 0 meets the reference's stop test (||r|| <= tol) without a re-entry round both ways and the sweep counts
differ by at most one.
usage: python tools/x_tile_f32_proto.py [2.5nm|7.5nm ...]"""
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import blockcg_proto as bp  # noqa: E402
import precond_block_proto as pp  # noqa: E402
from oracle import oracle as oc  # noqa: E402


def neighbour_pattern(o, m):
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
    return Pn.tocsr()


def run(name, s=16, d=8, tol=1e-6):
    As, bs, sc, o = bp.system(name)
    m = As.shape[0]
    An = As.multiply(neighbour_pattern(o, m)).tocsr()
    At = (As - An).tocsr(); At.eliminate_zeros()
    N = (sp.identity(m, format="csr") - An).tocsr(); N.eliminate_zeros()
    # the stored values are the UNSCALED entries of X: round those, scale afterwards (one rounded value serves both triangles: At is symmetric and so
    # is its image)
    isc = sp.diags(1.0 / sc); Xt = (isc @ At @ isc).tocsr()
    Xt32 = Xt.copy(); Xt32.data = Xt32.data.astype(np.float32).astype(np.float64)
    At32 = (sp.diags(sc) @ Xt32 @ sp.diags(sc)).tocsr()
    A32 = (An + At32).tocsr()
    nrm = lambda M: np.sqrt((M.data ** 2).sum())
    print("%s: %d rows; neighbour part %d nnz, tunnelling part %d nnz; ||At||_F / ||An||_F = %.2e; ||At32 - At||_F / ||A||_F = %.2e; asymmetry of At32 %.1e"
          % (name, m, An.nnz, At.nnz, nrm(At) / nrm(An), nrm((At32 - At).tocsr()) / nrm(As), abs(At32 - At32.T).max()), flush=True)
    y0 = np.zeros(m)
    out = {}
    for tag, Aloop in (("fp64 tiles", As), ("fp32 tiles", A32)):
        op = pp.SplitOp(Aloop, N, d)
        opt = pp.SplitOp(As, N, d)
        bh = op.L(bs)
        t0 = time.time()
        yh, its = bp.bcg(op, bh, y0, s, tol=tol / 1.5)
        y = op.L(yh)
        true_r = np.linalg.norm(As @ y - bs)                   # fp64 operator, as the solve's final pass
        pre_r = np.linalg.norm(opt @ yh - bh)                  # fp64 residual of L A L (what the loop's stop test estimates)
        out[tag] = (y, its, true_r)
        print("  %s: %3d sweeps; true fp64 residual of column 0 %.3e (stop test %.0e: %s, re-entry %s); fp64 residual of L A L %.3e  [%.0f s]"
              % (tag, its, true_r, tol, "met" if true_r <= tol else "MISSED", "no" if true_r <= tol else "YES", pre_r, time.time() - t0), flush=True)
    (y64, i64, r64), (y32, i32, r32) = out["fp64 tiles"], out["fp32 tiles"]
    dy = np.linalg.norm(y32 - y64) / np.linalg.norm(y64)
    ok = r64 <= tol and r32 <= tol and abs(i64 - i32) <= 1
    print("  |delta solution| / |solution| = %.3e; sweeps %d vs %d: %s" % (dy, i64, i32, "PASS" if ok else "FAIL"), flush=True)
    return ok


if __name__ == "__main__":
    names = sys.argv[1:] or ["2.5nm", "7.5nm"]
    res = [run(n) for n in names]
    print("prototype: %s" % ("PASS" if all(res) else "FAIL"))
    sys.exit(0 if all(res) else 1)
