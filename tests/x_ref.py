"""Host reference of the current-solve matrix X on atom arrays: a numpy restatement of the operator stated in csrc/xshared.h (k_atom_rows,
tunnel_kind, wkb_T, x_entry, k_xval) and of the sub-block census of csrc/xt.hip (k_xt_census).  No project code in it; not a test module.

Decisions are taken in float64, operation by operation as the kernels state them: the compaction of the sites to atoms, the class flags with both
inner-contact windows (AF_MP_PAT, bound Na; AF_MP_VAL, bound Na + 2), membership of S (a < Na - 1), the ground atom dropped from the neighbour
rows, fabs(cba - cbb) > tol, dist < nn_dist (both forms of site_dist, C's round), the sign of E2 and the level sequence of wkb_T (iv += dE summed
in float64 decides how many levels an entry integrates).  Values are np.longdouble (64-bit significand here, asserted below): the WKB factors of
both kinds and both branches, the direct terms, rows 0 and 1, and the diagonal as the ground term minus the sum of the off-diagonals.

Every member of S is a vacancy or an inner-contact metal of the NARROW window, which lies inside the wide one, so between two members the class
part of tunnel_kind always holds and the kind is 1 for a (vacancy, metal) pair and 2 otherwise.  The reference still evaluates the flags as the
kernels do and does not use this.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "np.longdouble is no wider than float64 on this platform: the reference would not be one"

Q = 1.60217663e-19                   # csrc/common.h
HBAR = 1.054571817e-34
DEFECT, OXYGEN_DEFECT, VACANCY = 0, 1, 2
AF_V, AF_MP_PAT, AF_MP_VAL, AF_METAL, AF_CVAC = 1, 2, 4, 8, 16
XT_R, XT_C, XT_SBW = 32, 256, 32
U = 2.0 ** -53


def c_round(v):
    """C's round(): halves away from zero (np.round goes to even)"""
    t = np.trunc(v)
    return t + np.sign(v) * (np.abs(v - t) >= 0.5)


def site_dist(x1, y1, z1, x2, y2, z2, laty, latz, pbc, dtype=np.float64):
    """csrc/common.h: site_dist.  The image chosen (round) is a float64 decision in either dtype."""
    if pbc:
        fy = (np.asarray(y1) - y2) / laty; fz = (np.asarray(z1) - z2) / latz
        ny, nz = c_round(fy), c_round(fz)
        X1, Y1, Z1, X2, Y2, Z2 = (np.asarray(v, dtype=dtype) for v in (x1, y1, z1, x2, y2, z2))
        dx = X1 - X2
        gy = (Y1 - Y2) / dtype(laty) - ny.astype(dtype); gz = (Z1 - Z2) / dtype(latz) - nz.astype(dtype)
        dy, dz = gy * dtype(laty), gz * dtype(latz)
        return np.sqrt(dx * dx + dy * dy + dz * dz)
    X1, Y1, Z1, X2, Y2, Z2 = (np.asarray(v, dtype=dtype) for v in (x1, y1, z1, x2, y2, z2))
    dx, dy, dz = X2 - X1, Y2 - Y1, Z2 - Z1
    return np.sqrt(dx * dx + dy * dy + dz * dz)


def level_sequence(n=4096):
    """iv of wkb_T's loop: 0, then += dE in float64, one addition at a time"""
    dE = Q * 0.01
    iv = np.empty(n)
    v = 0.0
    for k in range(n):
        iv[k] = v
        v += dE
    return iv


_IV = level_sequence()


def pow15(e):
    return e * np.sqrt(e)


def pow15_quotient(E1, E2):
    """(E1^1.5 - E2^1.5) / (E1 - E2) for E1 > E2 >= 0 without the cancellation of the two powers: (E1^2 + E1 E2 + E2^2) / (E1^1.5 + E2^1.5).  The
    kernels form the difference of the powers and divide by a difference recomputed from E2; the reference evaluates the same real function at the
    same inputs, and that cancellation is what the measured R_KIND of x_cases.py consists of."""
    return (E1 * E1 + E1 * E2 + E2 * E2) / (pow15(E1) + pow15(E2))


def tunnel_kind(fa, fb, cba, cbb, tol, mpbit):
    v1, v2 = (fa & AF_V) != 0, (fb & AF_V) != 0
    m1, m2 = (fa & mpbit) != 0, (fb & mpbit) != 0
    t2t, c2t, c2c = v1 & v2, (v1 & m2) | (v2 & m1), m1 & m2
    ok = (t2t | c2t | c2c) & (np.abs(cba - cbb) > tol)
    return np.where(ok, np.where(c2t, 1, 2), 0)


def wkb_values(kind, dist_f64, cba, cbb, m_e, V0, dist_ld=None, inclusive=False):
    """T >= 0 of wkb_T for arrays of entries (kind 1 or 2 each), in longdouble.  dist in metres.  Returns (T, levels, branch): levels = terms of
    the kind-1 integral (0 for kind 2), branch = 1 where an E2 > 0 term was taken, 2 where an E2 < 0 term was, 3 where both (kind 1 only).
    inclusive: the level loop run with iv <= drop (a seeded fault for the CPU tests; never the contract)."""
    kind = np.asarray(kind)
    n = len(kind)
    drop64 = np.abs(np.asarray(cba, dtype=np.float64) - np.asarray(cbb, dtype=np.float64))
    drop = np.abs(np.asarray(cba, dtype=LD) - np.asarray(cbb, dtype=LD))
    dist = np.asarray(dist_f64 if dist_ld is None else dist_ld, dtype=LD)
    prefac = -(np.sqrt(LD(2) * LD(m_e)) / LD(HBAR)) * (LD(2) / LD(3))
    QV0 = LD(Q) * LD(V0)                                               # DKMC_Q * V0: both factors are float64 constants of the kernel
    QV0_64 = Q * V0
    T = np.zeros(n, dtype=LD); levels = np.zeros(n, dtype=np.int64); branch = np.zeros(n, dtype=np.int64)
    k2 = np.flatnonzero(kind == 2)
    if len(k2):
        E2_64 = QV0_64 - drop64[k2]
        E1, E2 = QV0, QV0 - drop[k2]
        pos, neg = E2_64 > 0, E2_64 < 0
        v = np.zeros(len(k2), dtype=LD)
        v[pos] = np.exp(prefac * dist[k2][pos] * pow15_quotient(E1, np.maximum(E2[pos], LD(0))))
        v[neg] = np.exp(prefac * (dist[k2][neg] / drop[k2][neg]) * pow15(E1))
        T[k2] = v; branch[k2] = np.where(pos, 1, np.where(neg, 2, 0))
    k1 = np.flatnonzero(kind == 1)
    if len(k1):
        assert drop64[k1].max() < _IV[-1]
        cnt = np.searchsorted(_IV, drop64[k1], side="right" if inclusive else "left")   # levels with iv < drop
        levels[k1] = cnt
        c1 = prefac * (dist[k1] / drop[k1])
        for L in np.unique(cnt):
            sel = np.flatnonzero(cnt == L)
            for lo in range(0, len(sel), 4096):
                s = sel[lo:lo + 4096]
                iv64 = _IV[:L][None, :]
                E1_64 = QV0_64 + iv64                                  # float64: the sign of E2 as the kernel sees it
                E2_64 = E1_64 - drop64[k1][s][:, None]
                E1 = QV0 + _IV[:L].astype(LD)[None, :]
                E2 = E1 - drop[k1][s][:, None]
                pos, neg = E2_64 > 0, E2_64 < 0
                arg = np.where(pos, drop[k1][s][:, None] * pow15_quotient(E1, np.where(pos, np.maximum(E2, LD(0)), LD(0))), pow15(E1))
                term = np.exp(c1[s][:, None] * arg)
                term = np.where(pos | neg, term, LD(0))
                T[k1[s]] = term.sum(axis=1)
                branch[k1[s]] = pos.any(axis=1) * 1 + neg.any(axis=1) * 2
    return T, levels, branch


def x_reference(element, charge, cb_edge, x, y, z, neigh, metals, n_src, n_gnd, nlc, pbc, laty, latz, nn_dist, tol, high_G, low_G, loop_G,
                m_e, V0, inclusive_levels=False):
    """Everything in SITE arrays as the GPU buffers hold them; neigh [N, nn] is the padded site neighbour index (input data, ascending rows).
    Returns a dict: Na, atom_site, flag, metal, S_atom (atom order), S_metals_first, nM, ns, the CSR (rp, ci, val longdouble, kind per entry:
    0 = columns 0 / 1 and the off-diagonals of rows 0 and 1, 1 = contact->trap, 2 = other tunnelling, 3 = direct, 4 = diagonal; row, diag_pos,
    offabs = sum |off-diagonals| per row, ground_term per atom), T [ns, ns] over S in ATOM order (longdouble, symmetric, zero diagonal, entries
    <= 0), pred [ns, ns] (the census predicate without the c > r part, atom order), levels / branch / kindT per T entry."""
    element = np.asarray(element); charge = np.asarray(charge)
    atom = (element != DEFECT) & (element != OXYGEN_DEFECT)
    atom_site = np.flatnonzero(atom)
    Na = len(atom_site); N_full = Na + 2; Nsub = Na + 1
    site_atom = np.full(len(element), -1, dtype=np.int64); site_atom[atom_site] = np.arange(Na)
    ael, aq = element[atom_site], charge[atom_site]
    acb = np.asarray(cb_edge, dtype=np.float64)[atom_site]
    ax, ay, az = (np.asarray(v, dtype=np.float64)[atom_site] for v in (x, y, z))
    a = np.arange(Na)
    metal = np.isin(ael, list(metals))
    vac = ael == VACANCY
    lo = (nlc - 1) * n_src
    mp_pat = metal & (a > lo) & (a < Na - (nlc - 1) * n_gnd)
    mp_val = metal & (a > lo) & (a < N_full - (nlc - 1) * n_gnd)
    flag = vac * AF_V + mp_pat * AF_MP_PAT + mp_val * AF_MP_VAL + metal * AF_METAL + (vac & (aq == 0)) * AF_CVAC
    inS = (a < Na - 1) & (vac | mp_pat)
    S = np.flatnonzero(inS); ns = len(S)
    isM = ~vac[S]
    S_mf = np.concatenate([S[isM], S[~isM]]); nM = int(isM.sum())
    # neighbour rows in atom numbering, the ground atom removed
    nb_rows = []
    neigh = np.asarray(neigh)
    for i in atom_site:
        r = neigh[i]; r = site_atom[r[r >= 0]]; r = r[(r >= 0) & (r != Na - 1)]
        nb_rows.append(r)
    # ---- tunnelling block over S (atom order) --------------------------------------------------------------------------------------------
    sx, sy, sz, scb, sf = ax[S], ay[S], az[S], acb[S], flag[S]
    I, J = np.triu_indices(ns, 1)
    d64 = site_dist(sx[I], sy[I], sz[I], sx[J], sy[J], sz[J], laty, latz, pbc)
    near = d64 < nn_dist
    kind_val = tunnel_kind(sf[I], sf[J], scb[I], scb[J], tol, AF_MP_VAL)
    kind_pat = tunnel_kind(sf[I], sf[J], scb[I], scb[J], tol, AF_MP_PAT)
    listed = np.zeros(len(I), dtype=bool)                            # pairs of the neighbour LIST (what the pattern kernel looks at)
    srank = np.full(Na, -1, dtype=np.int64); srank[S] = np.arange(ns)
    if ns > 1:
        lin = I * ns + J
        for r, i in enumerate(S):
            c = srank[nb_rows[i]]; c = c[c > r]
            if len(c):
                listed[np.searchsorted(lin, r * ns + c)] = True
    live = (kind_val != 0) & ~near
    T = np.zeros((ns, ns), dtype=LD); levels = np.zeros((ns, ns), dtype=np.int64); branch = np.zeros((ns, ns), dtype=np.int64)
    kindT = np.zeros((ns, ns), dtype=np.int64)
    if live.any():
        e = np.flatnonzero(live)
        dld = site_dist(sx[I[e]], sy[I[e]], sz[I[e]], sx[J[e]], sy[J[e]], sz[J[e]], laty, latz, pbc, dtype=LD)
        t, lv, br = wkb_values(kind_val[e], 1e-10 * d64[e], scb[I[e]], scb[J[e]], m_e, V0, dist_ld=LD(1e-10) * dld, inclusive=inclusive_levels)
        for M, v in ((T, -t), (levels, lv), (branch, br), (kindT, kind_val[e])):
            M[I[e], J[e]] = v; M[J[e], I[e]] = v
    pred = np.zeros((ns, ns), dtype=bool); pred[I, J] = live; pred[J, I] = live
    pat = np.zeros((ns, ns), dtype=bool); pp = (kind_pat != 0) & ~listed; pat[I, J] = pp; pat[J, I] = pp
    assert not (pp & near).any() and not (listed & ~near).any()   # the neighbour list and the distance test agree on every pair of S
    # ---- CSR: pattern and values -----------------------------------------------------------------------------------------------------------
    g = Na - 1
    dg = site_dist(ax, ay, az, ax[g], ay[g], az[g], laty, latz, pbc)
    rows_c, rows_v, rows_k = [], [], []
    c0 = np.concatenate([[0, 1], np.arange(max(N_full - n_gnd + 1, 2), N_full - 1)]).astype(np.int64)
    v0 = np.where(c0 == 0, LD(high_G), np.where(c0 == 1, -LD(loop_G), LD(0))); v0 = np.where(c0 > N_full - n_gnd, -LD(high_G), v0)
    rows_c.append(c0); rows_v.append(v0.astype(LD)); rows_k.append(np.where(c0 == 0, 4, 0))
    c1 = np.arange(n_src + 2, dtype=np.int64)
    v1 = np.where(c1 == 0, -LD(loop_G), LD(0)); v1 = np.where((c1 >= 2) | (c1 > N_full - n_gnd), -LD(high_G), v1)
    rows_c.append(c1); rows_v.append(v1.astype(LD)); rows_k.append(np.where(c1 == 1, 4, 0))
    for i in range(2, Nsub):
        at = i - 2
        nb = nb_rows[at]
        dnb = site_dist(ax[at], ay[at], az[at], ax[nb], ay[nb], az[nb], laty, latz, pbc)
        assert np.all(dnb < nn_dist)                                  # x_entry decides "direct" by distance: the listed neighbours are within it
        mm = metal[at] & metal[nb]; cc = bool(flag[at] & AF_CVAC) & ((flag[nb] & AF_CVAC) != 0)
        vnb = np.where(mm | cc, -LD(high_G), -LD(low_G)).astype(LD)
        cols = [nb + 2, np.array([i])]; vals = [vnb, np.array([LD(high_G) if dg[at] < nn_dist else LD(0)])]
        kinds = [np.full(len(nb), 3), np.array([4])]
        r = srank[at]
        if r >= 0:
            tc = np.flatnonzero(pat[r])
            cols.append(S[tc] + 2); vals.append(T[r, tc]); kinds.append(kindT[r, tc])
        cols = np.concatenate(cols); vals = np.concatenate(vals); kinds = np.concatenate(kinds)
        o = np.argsort(cols, kind="stable")
        cols, vals, kinds = cols[o], vals[o], kinds[o]
        assert np.all(np.diff(cols) > 0)
        pre_c, pre_v = [], []
        if i > N_full - n_gnd: pre_c.append(0); pre_v.append(-LD(high_G))
        if i < n_src + 2: pre_c.append(1); pre_v.append(-LD(high_G))
        rows_c.append(np.concatenate([np.array(pre_c, dtype=np.int64), cols]))
        rows_v.append(np.concatenate([np.array(pre_v, dtype=LD), vals]))
        rows_k.append(np.concatenate([np.zeros(len(pre_c), dtype=np.int64), kinds]))
    cnt = np.array([len(c) for c in rows_c])
    rp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    ci = np.concatenate(rows_c); val = np.concatenate(rows_v).astype(LD); kind = np.concatenate(rows_k)
    rowid = np.repeat(np.arange(Nsub), cnt)
    dpos = np.flatnonzero(kind == 4)
    assert len(dpos) == Nsub and np.array_equal(ci[dpos], np.arange(Nsub))
    off = np.zeros(Nsub, dtype=LD); np.add.at(off, rowid[kind != 4], val[kind != 4])
    offabs = np.zeros(Nsub, dtype=LD); np.add.at(offabs, rowid[kind != 4], np.abs(val[kind != 4]))
    val[dpos] = val[dpos] - off
    return dict(Na=Na, atom_site=atom_site, flag=flag, metal=metal, S_atom=S, S_metals_first=S_mf, nM=nM, ns=ns, rp=rp, ci=ci, val=val,
                kind=kind, row=rowid, diag_pos=dpos, offabs=offabs, T=T, pred=pred, levels=levels, branch=branch, kindT=kindT, ground_term=dg < nn_dist)


def census(pred):
    """Sub-block masks of k_xt_census over S in the order pred is given in: bit q of cell (k, w) is set when a pair (r, c), c > r, of the rows
    32 k ... and the columns 256 w + 32 q ... passes the predicate.  Returns masks [nK, nW] and the upper-triangle predicate."""
    ns = pred.shape[0]
    nK, nW = (ns + XT_R - 1) // XT_R, (ns + XT_C - 1) // XT_C
    up = np.triu(pred, 1)
    P = np.zeros((nK * XT_R, nW * XT_C), dtype=bool); P[:ns, :ns] = up
    blocks = P.reshape(nK, XT_R, nW, XT_C // XT_SBW, XT_SBW).any(axis=(1, 4))          # [nK, nW, 8]
    masks = (blocks * (1 << np.arange(XT_C // XT_SBW))[None, None, :]).sum(axis=2).astype(np.int64)
    return masks, up


def tile_values(T, up, k, w, q):
    """the 32 x 32 doubles a stored sub-block must hold: T where the pair passes, 0.0 elsewhere and beyond ns"""
    ns = T.shape[0]
    out = np.zeros((XT_R, XT_SBW), dtype=LD)
    r0, c0 = XT_R * k, XT_C * w + XT_SBW * q
    r1, c1 = min(r0 + XT_R, ns), min(c0 + XT_SBW, ns)
    if r1 > r0 and c1 > c0:
        out[:r1 - r0, :c1 - c0] = np.where(up[r0:r1, c0:c1], T[r0:r1, c0:c1], LD(0))
    return out
