"""Host reference of the potential matrix K (background potential, CB edge): patterns, link classes, diagonal, right-hand side, one product and the
solution, from the neighbour index alone.  numpy / scipy only, np.longdouble values; shares no code with the library or the CPU oracle.  Pinned
against the oracle by tests/test_k_ref.py before tests/test_gpu_k_synthetic.py trusts it.  Not a test module.

Rows of K are the sites N_left <= i < N - N_left (m of them).  Rule 0 is the potential, rule 1 the CB edge, rule 2 the CB edge on atoms only.
Every decision (which block an entry belongs to, whether a link exists, its class) is taken on integers; only then do values appear:
    w_ij = high_G or low_G          diag_i = sum_j w_ij over the row's links to device sites and to both contacts
    rhs_i = kl_i VL + kr_i VR       kl / kr: the sums of the row's links to the left / right contact
The sums are formed as (count of high links) high_G + (count of low links) low_G in longdouble: two products and one addition per quantity.
Quirks of the solver that the reference does not share and the tests only document: the first stop test of the CG is on ||r|| (not ||r||^2)
against tol^2; a site without any link under rules 0 and 1 has a zero diagonal (1 / sqrt(0) in the Jacobi scaling) -- no case contains one."""
import numpy as np

LD = np.longdouble
DEFECT, OXYGEN_DEFECT, VACANCY = 0, 1, 2
NOLINK, LOW, HIGH = 0, 1, 2


def charges(neigh, element, charge, metals):
    """the charge rule: a vacancy is neutral next to a metal or to two vacancies, else +2; an oxygen interstitial is neutral next to a metal,
    else -2; every other site keeps the charge it has"""
    element = np.asarray(element); nb = np.asarray(neigh)
    ok = nb >= 0
    en = element[np.where(ok, nb, 0)]
    metal = (np.isin(en, metals) & ok).any(axis=1)
    nvac = ((en == VACANCY) & ok).sum(axis=1)
    out = np.array(charge, dtype=np.int32, copy=True)
    v, od = element == VACANCY, element == OXYGEN_DEFECT
    out[v] = np.where(metal[v] | (nvac[v] >= 2), 0, 2)
    out[od] = np.where(metal[od], 0, -2)
    return out


def _csr(rows, cols, m):
    rp = np.zeros(m + 1, dtype=np.int64); np.add.at(rp, rows + 1, 1)
    return np.cumsum(rp), cols.astype(np.int64)


def patterns(neigh, N_left):
    """The three CSR blocks over the rows of K, entries in the order of the neighbour row: device block (columns relative to N_left, the diagonal
    inserted in front of the first device neighbour above the row's own site, or at the end), device x left contact (site numbers), device x right
    contact (columns relative to N_left + m).  Returns ((rp, ci), (lrp, lci), (rrp, rci)) and the sites (global numbers) behind every entry."""
    nb = np.asarray(neigh, dtype=np.int64)
    N, nn = nb.shape
    m = N - 2 * N_left
    nb = nb[N_left:N_left + m]
    site = N_left + np.arange(m)[:, None]
    ok = nb >= 0
    left, right = ok & (nb < N_left), ok & (nb >= N_left + m)
    dev = ok & ~left & ~right
    above = dev & (nb > site)
    first = np.where(above.any(axis=1), above.argmax(axis=1), nn)               # slot the diagonal goes in front of
    r, s = np.nonzero(dev)
    key = np.concatenate([r * (2 * nn + 2) + 2 * s + 1, np.arange(m) * (2 * nn + 2) + 2 * first])
    rows = np.concatenate([r, np.arange(m)]); sites = np.concatenate([nb[r, s], N_left + np.arange(m)])
    o = np.argsort(key, kind="stable")
    P = _csr(rows[o], sites[o] - N_left, m)
    rl, sl = np.nonzero(left); rr, sr = np.nonzero(right)
    Pl = _csr(rl, nb[rl, sl], m); Pr = _csr(rr, nb[rr, sr] - (N_left + m), m)
    return (P, Pl, Pr), (sites[o], nb[rl, sl], nb[rr, sr])


def link(rule, ei, ej, qi, qj, metals):
    """class of the link between sites of elements ei, ej and charges qi, qj: NOLINK, LOW or HIGH (integer arrays in, integer array out)"""
    m1, m2 = np.isin(ei, metals), np.isin(ej, metals)
    if rule == 0:
        cv1, cv2 = (ei == VACANCY) & (qi == 0), (ej == VACANCY) & (qj == 0)
        return np.where((m1 & m2) | (cv1 & cv2), HIGH, LOW)
    out = np.where(m1 | m2, HIGH, LOW)
    if rule == 2:
        inter = (ei == DEFECT) | (ei == OXYGEN_DEFECT) | (ej == DEFECT) | (ej == OXYGEN_DEFECT)
        out = np.where(inter, NOLINK, out)
    return out


def system(neigh, element, charge, metals, N_left, high_G, low_G, VL, VR, rule):
    """K and its right-hand side.  rp / ci: the device block; cls: class of every entry (NOLINK on the diagonal position); val: the entry in
    longdouble (diagonal included, off-diagonals negative); diag, rhs, kl, kr; nterm: links of the row (device + both contacts), nrhs: links to the
    contacts, nprod: terms of the row in a product (its device links and the diagonal); rhs_abs = |kl VL| + |kr VR|; identity: rows that rule 2 left without a link (diagonal 1, rhs 0)."""
    element = np.asarray(element, dtype=np.int64); charge = np.asarray(charge, dtype=np.int64)
    (P, Pl, Pr), (sj, sl, sr) = patterns(neigh, N_left)
    m = len(P[0]) - 1
    H, Lo = LD(high_G), LD(low_G)
    cnt = {}
    classes = []
    for (rp, _), js in zip((P, Pl, Pr), (sj, sl, sr)):
        rows = np.repeat(np.arange(m), np.diff(rp))
        i = N_left + rows
        c = link(rule, element[i], element[js], charge[i], charge[js], metals)
        c = np.where(js == i, NOLINK, c)
        classes.append(c)
        cnt[len(classes)] = (np.bincount(rows[c == HIGH], minlength=m), np.bincount(rows[c == LOW], minlength=m))
    wsum = lambda k: cnt[k][0].astype(LD) * H + cnt[k][1].astype(LD) * Lo
    off, kl, kr = wsum(1), wsum(2), wsum(3)
    diag = off + kl + kr
    nterm = sum(cnt[k][0] + cnt[k][1] for k in (1, 2, 3))
    identity = nterm == 0
    if rule == 2:
        diag = np.where(identity, LD(1), diag)
    rhs = kl * LD(VL) + kr * LD(VR)
    rp, ci = P
    rows = np.repeat(np.arange(m), np.diff(rp))
    cls = classes[0]
    val = np.where(cls == HIGH, -H, np.where(cls == LOW, -Lo, LD(0)))
    val = np.where(ci == rows, diag[rows], val)
    return dict(m=m, N_left=N_left, rule=rule, rp=rp, ci=ci, rows=rows, cls=cls, val=val, lrp=Pl[0], lci=Pl[1], rrp=Pr[0], rci=Pr[1],
                cls_left=classes[1], cls_right=classes[2], diag=diag, rhs=rhs, kl=kl, kr=kr, nterm=nterm, nprod=cnt[1][0] + cnt[1][1] + 1,
                nrhs=cnt[2][0] + cnt[2][1] + cnt[3][0] + cnt[3][1], rhs_abs=np.abs(kl * LD(VL)) + np.abs(kr * LD(VR)), identity=identity,
                offdiag=np.diff(rp) - 1)


def product(S, v, absolute=False):
    """K v in longdouble (every row of the device block holds its diagonal, so no segment of the reduction is empty); absolute: sum_j |k_ij v_j|"""
    terms = S["val"] * np.asarray(v, dtype=LD)[S["ci"]]
    return np.add.reduceat(np.abs(terms) if absolute else terms, S["rp"][:-1])


def scaled_residual(S, y):
    """|| D^-1/2 (K y - b) ||_2 in longdouble: the residual of the Jacobi-scaled system the CG iterates on, at the unscaled y"""
    r = (product(S, y) - S["rhs"]) / np.sqrt(S["diag"])
    return float(np.sqrt((r * r).sum()))


def matrix(S):
    """K rounded to float64 (scipy CSR)"""
    import scipy.sparse as sp
    return sp.csr_matrix((S["val"].astype(np.float64), S["ci"], S["rp"]), shape=(S["m"], S["m"]))


def solve(S, rounds=12):
    """y with K y = rhs: a float64 sparse LU of K, refined with the longdouble residual until the scaled residual stops falling.  Returns
    (y in longdouble, its scaled residual), which is asserted to be at most 1e-16."""
    import scipy.sparse.linalg as spl
    lu = spl.splu(matrix(S).tocsc())
    y = np.zeros(S["m"], dtype=LD)
    best, ybest = np.inf, y
    for _ in range(rounds):
        y = y - lu.solve((product(S, y) - S["rhs"]).astype(np.float64)).astype(LD)
        res = scaled_residual(S, y)
        if not res < best:
            break
        best, ybest = res, y
    assert best <= 1e-16, best
    return ybest, best
