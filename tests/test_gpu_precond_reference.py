"""The split polynomial preconditioner L = p(N) of the block-CG (csrc/xtb_precond.h: k_xtb_nmul, k_xtb_npack*, k_xtb_nmulp, k_xtb_qs_from, xtb_applyL)
against a plain long-double reference of the same operation.  The loop only sees "another SPD operator" and re-enters on its true residual,
so a wrong L shows up as more sweeps at most; these tests compare L itself.

Every comparison is element by element:  |gpu - ref| <= c u B,  u = 2^-53, B the same computation with every term in absolute value and c a
small count of roundings stated next to it (never looser than 1e-12 B).  Every group carries a negative control that the same assertion rejects.

a. One Horner step out = ca add + cb (N in) (dkmc_xtb_test_nstep) over synthetic CSR matrices that reach every branch of both kernels: row
   lengths around the 4 / 8 / 12 / 16-slot batches and the 64-entry rounds, filtered entries (driver columns, the diagonal), driver rows with
   entries of their own, unsorted and duplicate columns, an empty slice of four rows, row counts below, at and off multiples of the 8-block map.
b. The full L with QS on the X of a real solve (dkmc_xtb_check_poly) against N built independently from the exported CSR and the site
   neighbour list."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import params_7p5
from devicekmc_amd.lib import check
from test_gpu_parity import Vd, _fresh_device, get, hip  # noqa: F401

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _ok(gpu, ref, B, c):
    """Element-wise |gpu - ref| <= c u B (NaN fails)."""
    assert np.all(c * U <= 1e-12)
    return np.abs(gpu.astype(LD) - ref) <= LD(c * U) * B


# ---- a. one Horner step on synthetic N -----------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130, 200]


def _synthetic(m, seed):
    """CSR (rp int64, ci, val), sc, in, add of m rows: every row length of LENGTHS (small m: as many as fit), columns 0 / 1 and the diagonal
    among the entries (outside N), a duplicate column in most rows, unsorted columns, driver rows 0 / 1 with entries, rows 8 ... 11 empty."""
    rng = np.random.default_rng(seed)
    if m > 100000:
        ln = rng.integers(0, 7, m)
        ln[::997] = np.resize(LENGTHS, len(ln[::997]))
    else:
        ln = np.resize(np.roll(LENGTHS, seed % len(LENGTHS)), m)
    ln[0], ln[1] = 5, 17
    if m >= 12:
        ln[8:12] = 0                                                  # slice 2: four empty rows
    rp = np.zeros(m + 1, dtype=np.int64); rp[1:] = np.cumsum(ln)
    nnz = int(rp[-1])
    row = np.repeat(np.arange(m), ln)
    ci = rng.integers(0, m, nnz).astype(np.int32)
    pos = np.arange(nnz) - rp[row]
    kind = rng.integers(0, 10, nnz)
    ci[kind == 0] = 0                                                 # driver columns
    ci[kind == 1] = 1
    ci[kind == 2] = row[kind == 2]                                    # the diagonal
    dup = (pos == 1) & (ln[row] >= 3)
    ci[dup] = ci[np.flatnonzero(dup) - 1]                             # a duplicate column
    val = rng.uniform(-1.0, 1.0, nnz)
    sc = rng.uniform(0.5, 2.0, m)
    vin = rng.standard_normal((m, 16))
    add = rng.standard_normal((m, 16))
    return rp, ci, val, sc, vin, add


def _step_reference(m, rp, ci, val, sc, vin, add, ca, cb, drop=None):
    """out_r = ca add_r - cb sc_r sum val sc_c in_c (c >= 2, c != r; rows 0 / 1: ca add), its bound B and the roundings c of every row.
    drop: index of one entry to leave out (negative control)."""
    row = np.repeat(np.arange(m), np.diff(rp))
    keep = (ci >= 2) & (ci != row) & (row >= 2)
    if drop is not None:
        keep[drop] = False
    w = val[keep].astype(LD) * sc[ci[keep]].astype(LD)
    M = sp.csr_matrix((w, (row[keep], ci[keep])), shape=(m, m), dtype=LD)
    Ma = sp.csr_matrix((np.abs(w), (row[keep], ci[keep])), shape=(m, m), dtype=LD)
    x = vin.astype(LD)
    scr = sc.astype(LD)[:, None]
    ref = LD(ca) * add.astype(LD) - LD(cb) * scr * (M @ x)
    B = np.abs(LD(ca) * add.astype(LD)) + abs(LD(cb)) * scr * (Ma @ np.abs(x))
    # roundings of a row of k entries: k products val sc_c (folded into one with in_c: 2 each), the k-term sum in four accumulators, then
    # sc_r, cb, ca add and the difference -- 2 k + 6 bounds them all
    c = 2 * np.diff(rp).astype(np.int64) + 6
    return ref, B, c[:, None]


def _nstep(L, m, rp, ci, val, sc, vin, add, ca, cb, form, rowlist=None, nsrank=None, ns=0):
    out = np.full((m, 16), np.nan)
    qs = np.zeros((max(ns, 1), 16)) if nsrank is not None else None
    check(L.dkmc_xtb_test_nstep(m, _p(rp), _p(ci), _p(val), _p(sc), _p(vin), _p(add), ca, cb, form, _p(rowlist),
                                0 if rowlist is None else len(rowlist), _p(nsrank), ns, _p(out), _p(qs)))
    return out, qs


@pytest.mark.parametrize("m", [3, 4, 5, 17, 63, 64, 65, 129, 1000003])
def test_horner_step_on_synthetic_n(hip, m):
    host, L = hip
    rp, ci, val, sc, vin, add = _synthetic(m, seed=m)
    rng = np.random.default_rng(m + 1)
    # S ranks: a random half of the rows (drivers included), in a random order
    srows = rng.permutation(np.flatnonzero(rng.random(m) < 0.5))
    nsrank = np.full(m, -1, dtype=np.int32); nsrank[srows] = np.arange(len(srows), dtype=np.int32)
    ns = len(srows)
    # row list: shuffled, non-contiguous, rows 0 / 1 in it, a length that is not a multiple of 4
    lst = np.flatnonzero(rng.random(m) < 0.6)
    lst = np.union1d(lst, [0, 1])
    if len(lst) % 4 == 0:
        lst = lst[:-1] if len(lst) > 3 else lst[:3]
    rowlist = rng.permutation(lst).astype(np.int32)
    listed = np.zeros(m, dtype=bool); listed[rowlist] = True
    pairs = [(0.7182818284590452, 1.0), (-1.3125, 0.6180339887498949)] if m < 100000 else [(-1.3125, 0.6180339887498949)]
    checked = 0
    for ca, cb in pairs:
        ref, B, c = _step_reference(m, rp, ci, val, sc, vin, add, ca, cb)
        for lst_on in (False, True):
            outs = {}
            for form in (0, 1):
                out, qs = _nstep(L, m, rp, ci, val, sc, vin, add, ca, cb, form, rowlist if lst_on else None, nsrank if ns else None, ns)
                rows = listed if lst_on else np.ones(m, dtype=bool)
                good = _ok(out[rows], ref[rows], B[rows], c[rows])
                assert good.all(), (m, ca, lst_on, form, np.argwhere(~good)[:5])
                if lst_on:
                    assert np.isnan(out[~listed]).all(), (m, form)             # rows outside the list: untouched
                if ns:
                    sr = nsrank[rows]; r = np.flatnonzero(rows)[sr >= 0]
                    assert np.array_equal(qs[nsrank[r]], sc[r, None] * out[r]), (m, lst_on, form)
                outs[form] = out
                checked += 1
            assert outs[0].tobytes() == outs[1].tobytes(), (m, ca, lst_on)      # both forms: the same bits
    # negative control: the reference without one entry of N (the largest term of the longest row) is rejected by the same assertion
    row = np.repeat(np.arange(m), np.diff(rp))
    inN = (ci >= 2) & (ci != row) & (row >= 2)
    if inN.any():
        term = np.where(inN, np.abs(val * sc[ci] * vin[ci, 0]), -1.0)
        drop = int(np.argmax(term))
        ca, cb = pairs[-1]
        ref2, B2, c2 = _step_reference(m, rp, ci, val, sc, vin, add, ca, cb, drop=drop)
        out, _ = _nstep(L, m, rp, ci, val, sc, vin, add, ca, cb, 1)
        assert not _ok(out, ref2, B2, c2).all(), m
    else:
        assert m <= 3                                                    # (m = 3: every entry is a driver column or the diagonal)
    assert checked == 4 * len(pairs)


def test_nstep_refuses_columns_outside_the_rows(hip):
    host, L = hip
    rp = np.array([0, 0, 0, 1], dtype=np.int64); ci = np.array([3], dtype=np.int32); val = np.ones(1); sc = np.ones(3)
    vin = np.zeros((3, 16)); add = np.zeros((3, 16)); out = np.zeros((3, 16))
    assert L.dkmc_xtb_test_nstep(3, _p(rp), _p(ci), _p(val), _p(sc), _p(vin), _p(add), 1.0, 1.0, 1, None, 0, None, 0, _p(out), None) != 0
    L.dkmc_clear_error()


# ---- b. L on the X of a real solve ---------------------------------------------------------------------------------------------------------
DEGREES = [1, 2, 7, 8, 16]


def _coeffs(L, d):
    pc = np.zeros(17)
    check(L.dkmc_xtb_poly_coeffs(d, pc.ctypes.data_as(C.POINTER(C.c_double))))
    return pc[:d + 1]


def _split(dev, rp, ci, data, stats):
    """N = -S An S (neighbour couplings of atom rows >= 2, S = diag(X)^-1/2) from the exported CSR of X and the site neighbour list alone;
    checks that this classification accounts for every stored entry of the GPU's Xs and its tiles."""
    n = len(rp) - 1
    row = np.repeat(np.arange(n), np.diff(rp))
    diag = row == ci
    assert diag.sum() == n
    d = np.zeros(n); d[row[diag]] = data[diag]
    sc = 1.0 / np.sqrt(d)
    el = dev.site_element
    atom_site = np.flatnonzero((el != 0) & (el != 1))
    na = len(atom_site)
    assert n == na + 1
    site_atom = np.full(len(el), -1, dtype=np.int64); site_atom[atom_site] = np.arange(na)
    nb = dev.neigh_idx[atom_site]                                        # [na][nn] sites, -1 padded
    nba = np.where(nb >= 0, site_atom[np.maximum(nb, 0)], -1)
    a_of = np.repeat(np.arange(na), nb.shape[1])
    keys = np.unique((a_of * na + nba.ravel())[nba.ravel() >= 0])
    atom = (row >= 2) & (ci >= 2)
    neigh = atom & ~diag & np.isin((row - 2).astype(np.int64) * na + (ci - 2), keys)
    drv = ~diag & ~atom
    xs_nnz = stats["X_nnz"] - 2 * stats["spmv_tile_entries"]
    assert neigh.sum() + n + drv.sum() == xs_nnz, (neigh.sum(), n, drv.sum(), xs_nnz)
    assert (atom & ~diag & ~neigh).sum() == 2 * stats["spmv_tile_entries"]
    w = -(sc[row[neigh]].astype(LD) * data[neigh].astype(LD) * sc[ci[neigh]].astype(LD))
    N = sp.csr_matrix((w, (row[neigh], ci[neigh])), shape=(n, n), dtype=LD)
    Na = sp.csr_matrix((np.abs(w), (row[neigh], ci[neigh])), shape=(n, n), dtype=LD)
    kmax = int(np.bincount(row[neigh | diag | drv], minlength=n)[2:].max())  # stored entries of the longest atom row of Xs (rows 0 / 1 sum nothing)
    # the largest single term of N v (negative control: that entry dropped)
    return N, Na, sc, kmax, (row[neigh], ci[neigh], w)


def _poly_ref(N, Na, v, pc):
    """L v = sum_j c_j N^j v, its bound sum_j |c_j| |N|^j |v|, and the input of the last Horner step, sum_{j >= 1} c_j N^(j - 1) v."""
    P = v.astype(LD); A = np.abs(P)
    ref = LD(pc[0]) * P; B = abs(LD(pc[0])) * A; prev = np.zeros_like(P)
    for j in range(1, len(pc)):
        prev += LD(pc[j]) * P
        P = N @ P; A = Na @ A
        ref += LD(pc[j]) * P; B += abs(LD(pc[j])) * A
    return ref, B, prev


def _solve_once(structure, p, hip):
    host, L = hip
    dev, sim, gb, _ = _fresh_device(structure, p, hip)
    dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, 0); dev.updatePower(gb, p, Vd)
    return dev, gb


def _record(dev, gb, host):
    return dict(m=get(gb, "atom_virtual_potentials").copy(), im=np.float64(dev.imacro).tobytes(), iters=host.get_stats()["cg_iters_X"])


@pytest.mark.parametrize("which", ["2.5nm", "7.5nm"])
def test_poly_on_the_resident_x(cell_2p5, dev_7p5, hip, which):
    from devicekmc_amd import params as pm
    host, L = hip
    structure, mk = (cell_2p5, pm.KMCParameters) if which == "2.5nm" else (dev_7p5, params_7p5)
    assert L.dkmc_get_x_poly() == 8 and L.dkmc_get_x_block() == 16
    p = mk(); p.solve_heating_global = False
    dev, gb = _solve_once(structure, p, hip)
    first = _record(dev, gb, host)
    stats = host.get_stats()
    assert stats["xb_width"] == 16 and stats["xt_ns"] > 0
    rp, ci, data = host.get_last_X()
    N, Na, sc, kmax, (nr, nc, nw) = _split(dev, rp, ci, data, stats)
    n, ns = len(rp) - 1, stats["xt_ns"]
    v = np.random.default_rng(7).standard_normal((n, 16))
    # the S rows: every row of a tile entry is one; QS row q belongs to the row r whose sc_r (L v)_r it holds
    row = np.repeat(np.arange(n), np.diff(rp))
    tile_rows = np.unique(row[(row >= 2) & (ci >= 2) & (row != ci) & ~np.isin(row.astype(np.int64) * n + ci, nr.astype(np.int64) * n + nc)])
    srow = None
    for d in DEGREES:
        pc = _coeffs(L, d)
        ref, B, prev = _poly_ref(N, Na, v, pc)
        c = d * (2 * kmax + 8)                                           # d steps of at most 2 k + 6 roundings each (+ slack for |N| |y| vs B)
        outs = {}
        for form in (0, 1):
            out = np.full((n, 16), np.nan); qs = np.full((ns, 16), np.nan)
            check(L.dkmc_xtb_check_poly(d, form, _p(np.ascontiguousarray(v)), _p(out), _p(qs)))
            good = _ok(out, ref, B, c)
            print(which, "d", d, "form", form, "max |gpu - ref| / (u B) = %.2f of c = %d" % (float(np.max(np.abs(out.astype(LD) - ref) / (U * B))), c))
            assert good.all(), (which, d, form, np.argwhere(~good)[:5])
            if srow is None:
                # map QS rows to X rows through the GPU's own product (distinct random values: one match each)
                key = sc * out[:, 0]
                order = np.argsort(key); ks = key[order]
                hi = np.clip(np.searchsorted(ks, qs[:, 0]), 1, n - 1)
                pick = np.where(np.abs(ks[hi] - qs[:, 0]) <= np.abs(ks[hi - 1] - qs[:, 0]), hi, hi - 1)
                srow = order[pick]
                assert len(np.unique(srow)) == ns and srow.min() >= 2
                assert np.isin(tile_rows, srow).all()
            assert np.all(np.abs(qs - sc[srow, None] * out[srow]) <= 4 * U * np.abs(qs)), (which, d, form)
            qref = sc[srow, None].astype(LD) * ref[srow]; qB = sc[srow, None].astype(LD) * B[srow]
            assert _ok(qs, qref, qB, c + 2).all(), (which, d, form)
            # negative control (QS): the copy of the step before the last is rejected
            assert not _ok(qs, sc[srow, None].astype(LD) * prev[srow], qB, c + 2).all(), (which, d, form)
            outs[form] = out
        assert outs[0].tobytes() == outs[1].tobytes(), (which, d)
        out = outs[1]
        # negative controls (L): one c_j scaled by 1 + 1e-9, the degree-(d - 1) schedule
        j = int(np.argmax(np.abs(pc)))
        pj = pc.copy(); pj[j] *= 1 + 1e-9
        assert not _ok(out, _poly_ref(N, Na, v, pj)[0], B, c).all(), (which, d, "c_j")
        assert not _ok(out, _poly_ref(N, Na, v, pc[:d])[0], B, c).all(), (which, d, "degree d - 1")
        if d == 2:
            # negative control: N without its largest coupling
            k = int(np.argmax(np.abs(nw)))
            keep = np.ones(len(nw), dtype=bool); keep[k] = False
            N2 = sp.csr_matrix((nw[keep], (nr[keep], nc[keep])), shape=(n, n), dtype=LD)
            assert not _ok(out, _poly_ref(N2, Na, v, pc)[0], B, c).all(), (which, "dropped entry")
    # the aid leaves the next solve alone: a warm solve after it gives the bits of the same sequence without it
    dev.updatePower(gb, p, Vd)
    with_aid = _record(dev, gb, host)
    dev2, gb2 = _solve_once(structure, p, hip)
    first2 = _record(dev2, gb2, host)
    dev2.updatePower(gb2, p, Vd)
    without = _record(dev2, gb2, host)
    for a, b in ((first, first2), (with_aid, without)):
        assert a["m"].tobytes() == b["m"].tobytes() and a["im"] == b["im"] and a["iters"] == b["iters"], which


def test_check_poly_refuses_bad_arguments(cell_2p5, hip):
    host, L = hip
    from devicekmc_amd import params as pm
    p = pm.KMCParameters(); p.solve_heating_global = False
    _solve_once(cell_2p5, p, hip)
    n = len(host.get_last_X()[0]) - 1
    v = np.zeros((n, 16)); out = np.zeros((n, 16)); qs = np.zeros((host.get_stats()["xt_ns"], 16))
    for d, form in ((0, 1), (17, 1), (8, 2)):
        assert L.dkmc_xtb_check_poly(d, form, _p(v), _p(out), _p(qs)) != 0, (d, form)
        L.dkmc_clear_error()

