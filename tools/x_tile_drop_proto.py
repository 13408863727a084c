#!/usr/bin/env python3
"""CPU experiment behind dkmc_set_x_tile_drop: how much of the tunnelling block of the oracle's Jacobi-scaled X the sweeps could
ignore, and what ignoring it does to a warm-started solve.  On coupled oracle supersteps (CPU side only: nothing here touches the GPU):
  table 1 (first step): the share of the S x S off-diagonal entries with |a_ij| >= 1e-10 and >= 1e-12, of the stored 32 x 32 sub-blocks and of the
           stored 32 x 256 tiles (upper triangle, S in atom order: the layout of csrc/xt.hip) that hold any such entry;
  table 2 (every step): for theta = 1e-9 ... 1e-12, ||E y|| for the solution y of the step (what a COLD start would see) and ||E (y - y_prev)|| for the
           correction of a warm start from the previous step's solution, E = A - A~ with the entries below theta dropped one by one, and (a second
           line) with whole tiles dropped -- which removes less.  Beside them ||b||, ||y||, ||correction|| and the stop test.
Every solve runs the oracle's own Jacobi-scaled CG to 1e-10.
usage: python tools/x_tile_drop_proto.py [2.5nm|7.5nm|tile:K ...] [--steps 3]"""
import argparse
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import blockcg_proto as bp  # noqa: E402
import x_tile_f32_proto as fp  # noqa: E402
from oracle import oracle as oc  # noqa: E402

THETAS = (1e-9, 1e-10, 1e-11, 1e-12)
TOL = 1e-6


def scaled(o, p, Vd):
    X = o.last_X
    Na = X["Na"]; m = Na + 1
    A = sp.csr_matrix((X["data"], X["col"], X["row_ptr"][:m + 1]), shape=(m, Na + 2))[:, :m].tocsr()
    b = np.zeros(m); b[0] = -p.X_loop_G * Vd; b[1] = p.X_loop_G * Vd
    sc = 1.0 / np.sqrt(A.diagonal())
    return (sp.diags(sc) @ A @ sp.diags(sc)).tocsr(), b * sc, sc


def tunnelling_part(As, o):
    m = As.shape[0]
    An = As.multiply(fp.neighbour_pattern(o, m)).tocsr()
    At = (As - An).tocoo()
    keep = At.data != 0
    return At.row[keep], At.col[keep], np.abs(At.data[keep]), At.data[keep]


def tile_keys(r, c, rank):
    """sub-block and tile of every UPPER-triangle entry (S rank of the row below that of the column)"""
    i, j = rank[r], rank[c]
    up = j > i
    sub = (i[up] // 32).astype(np.int64) * (1 << 32) + j[up] // 32
    tile = (i[up] // 32).astype(np.int64) * (1 << 32) + j[up] // 256
    return up, sub, tile


def run(name, steps, Vd=5.0):
    s, p = bp.load(name)
    o = oc.OracleKMC(s.element, s.x, s.y, s.z, p)
    o.set_laplace_potential(Vd)
    xprev = None
    for step in range(1, steps + 1):
        o.superstep(Vd)
        As, bs, sc = scaled(o, p, Vd)
        m = As.shape[0]
        r, c, mag, val = tunnelling_part(As, o)
        members = np.unique(r)
        rank = np.full(m, -1, dtype=np.int64); rank[members] = np.arange(len(members))
        up, sub, tile = tile_keys(r, c, rank)
        if step == 1:
            nsub, ntile = len(np.unique(sub)), len(np.unique(tile))
            row = ["%s (%d rows, |S| = %d)" % (name, m, len(members))]
            row += ["%.2f" % (mag >= t).mean() for t in (1e-10, 1e-12)]
            row += ["%.2f" % (len(np.unique(sub[mag[up] >= t])) / nsub) for t in (1e-10, 1e-12)]
            row += ["%.2f" % (len(np.unique(tile[mag[up] >= 1e-10])) / ntile)]
            print("| | entries >= 1e-10 | >= 1e-12 | 32 x 32 sub-blocks with any entry >= 1e-10 | >= 1e-12 | 32 x 256 tiles with any entry >= 1e-10 |")
            print("| " + " | ".join(row) + " |", flush=True)
        y, its = bp.cg(As, bs, np.zeros(m) if xprev is None else xprev[:m] / sc, tol=1e-10)
        corr = None if xprev is None else y - xprev[:m] / sc
        print("step %d: ||b|| = %.1e, ||y|| = %.1e, ||correction|| = %s, stop test %.0e (%d CG iterations)"
              % (step, np.linalg.norm(bs), np.linalg.norm(y), "-" if corr is None else "%.2e" % np.linalg.norm(corr), TOL, its), flush=True)
        # the largest magnitude of every stored tile, handed back to its entries (both triangles of a pair live in the tile of the upper one)
        lo = rank[r] > rank[c]
        ti = np.where(lo, rank[c], rank[r]) // 32 * (1 << 32) + np.where(lo, rank[r], rank[c]) // 256
        order = np.argsort(ti, kind="stable"); tis = ti[order]
        first = np.r_[True, tis[1:] != tis[:-1]]
        tmax = np.maximum.reduceat(mag[order], np.flatnonzero(first))
        tmag = np.empty_like(mag); tmag[order] = np.repeat(tmax, np.diff(np.r_[np.flatnonzero(first), len(tis)]))
        for t in THETAS:
            line = "  theta %.0e:" % t
            for tag, dead in (("entries", mag < t), ("tiles", tmag < t)):
                E = sp.csr_matrix((val[dead], (r[dead], c[dead])), shape=(m, m))
                line += "  %s dropped %.2f: ||E y|| = %.1e" % (tag, dead.mean(), np.linalg.norm(E @ y))
                if corr is not None:
                    line += ", ||E correction|| = %.1e" % np.linalg.norm(E @ corr)
            print(line, flush=True)
        xprev = np.zeros(m + 8); xprev[:m] = y * sc                       # the unscaled solution: the next step's start vector


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=["tile:3"])
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    for n in a.workloads:
        run(n, a.steps)
