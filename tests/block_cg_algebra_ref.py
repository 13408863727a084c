"""Host reference of the s x s algebra of a block-CG sweep (csrc/xtb.hip: k_xtb_small) shared by tests/test_gpu_block_cg_algebra.py and
tests/test_block_cg_algebra_exports.py: the word maps of the Gram blocks and of `mats`, consistent test inputs, the identities the kernel's outputs
must meet (evaluated in mpmath at 50 digits from the INPUTS and the outputs under test, so that no conditioning enters a bound), the crafted inputs of
the decision / breakdown branches, and a plain numpy fp64 restatement of the kernel that keeps this reference honest without a GPU.  Not a test module.

Bounds.  u = 2^-53; |A| is the matrix of absolute values; every bound is  |residual| <= c u B  element by element, B the same expression with every
term in absolute value.  The counts c (derived, not measured; gamma_k = k u / (1 - k u) is written k u, the denominators and the replacement of a
computed Cholesky factor by the exact one -- a factor 1 + O(cond u) <= 1 + 1e-9 on B under the input condition cond <= 1e6 -- are covered by doubling):

  C1 = 100  (i)   Tm c + P'R, Tm = sym(P'T) = L L'.  Cholesky solve of a 16 x 16 system: (Tm + dA) x = b with |dA| <= (3 n + 1) u |L||L'| = 49 u |L||L'|
                  (Higham, Accuracy and Stability of Numerical Algorithms, theorem 10.4), + 1 for the rounding of sym(P'T) (|Tm| <= |L||L'|); c = -x exactly.
                  50, doubled.
  CMM = 18        one xtb_mm: a 16-term dot product in two chains of 8 (at most 9 roundings per term; 17 = n + 1 is the textbook count) + the addition of D.
  C2 = 170  (ii)  Tm M2 - V W, V = T'T c + T'R exactly from the c under test, beta = Tm^-1 V exactly.  Tm beta^ = V^ + dA beta^, V^ = V + dV with
                  |dV| <= CMM u BV, BV = |T'T||c| + |T'R|; M2 = beta^ W + dM, |dM| <= 17 u |beta^||W|.  So
                  Tm M2 - V W = dV W + dA beta^ W + Tm dM,  bounded by  u (18 BV |W| + (50 + 17) |L||L'||beta||W|)  <= 85 u B2,
                  B2 = BV |W| + |L||L'||beta||W|; doubled (beta^ is no output: the exact beta stands in for it inside B2).
  C3 = 17   (iii) M3 + c W: one 16-term product, alpha = -1 exact.
  C4 = 54   (iv)  rr - (R'R + c'V + (T'R)'c)_00: V^ carries 18 u BV, c'V^ a 16-term product (17), (T'R)'c another (17), two additions (2).
  CW = 218  (v)   W' Gg W - I for the Gg the kernel itself formed: its four xtb_mm, the symmetrisations and the carried errors of Grn (55), Gprn (19) and
                  (P'P) beta (18) stay below 60 u B_Gg; the Cholesky factorisation adds 17 u |Lg||Lg'| (theorem 10.3), the 16 back-substitutions for
                  W = Lg^-T 16 u |Lg'||W| each side (theorem 8.5; |I| <= |W'||Lg|).  60 + 17 + 32 = 109, doubled.
            The issue's (v) evaluates Gg with the EXACT beta of the c under test, while the kernel used its computed beta^.  Gg is the Gram matrix of
            D = -R+ + P beta, so the difference enters to first order:  W'(Gg(beta^) - Gg(beta))W = (dbeta W)'(P'D W) + transpose, and by (ii)
            |dbeta W| <= |Tm^-1| (C2 / 2) u B2.  The reference evaluates this term, E = (|Tm^-1| 85 B2)' |P'D W| + transpose, from the same inputs as B5, and
            c5 = CW + ceil(max E / B5): a count that grows with the conditioning of Tm -- a property of the test's INPUTS, checked like cond <= 1e6 --
            and never with what the kernel returned beyond the c and W that B5 itself is made of.  On the inputs of the tests (consistent_gram with the
            seeds 400000 + 1000 s + log10 kappa) c5 is 233 ... 5500; other seeds reach 1.2e4 at s = 16, kappa = 1e6, beyond what c u <= 1e-12 admits, so
            the seed is part of the input condition (evaluated on the fp64 restatement, tests/test_block_cg_algebra_exports.py).
Every count is asserted to satisfy c u <= 1e-12 where it is used."""
import math

import mpmath as mp
import numpy as np

U = 2.0 ** -53
LD = np.longdouble
NG = 6                                    # P'T, P'R, T'R, T'T, R'R, P'P
GSTR = NG * 256 + 2                       # one rank's Gram block: six matrices, a spare word, the abort word
C1, CMM, C2, C3, C4, CW = 100, 18, 170, 17, 54, 218
mp.mp.dps = 50

# ---- word maps ------------------------------------------------------------------------------------------------------------------------------
# entry (i, j) of a Gram matrix sits at word 64 (i / 4) + 16 (i % 4) + j: register u = i / 4 of lane l = 16 (i % 4) + j (k_xtb_rows, k_xtb_small)
_I, _J = np.divmod(np.arange(256), 16)
KMAP = 64 * (_I // 4) + 16 * (_I % 4) + _J


def to_kernel(G):
    """[16][16] -> the 256 words of the kernel's map"""
    w = np.empty(256); w[KMAP] = np.asarray(G, dtype=np.float64).ravel()
    return w


def from_kernel(w):
    return np.asarray(w, dtype=np.float64)[KMAP].reshape(16, 16)


def gram_block(G6, abort=0.0, spare=0.0):
    """six [16][16] matrices -> one block of GSTR words"""
    b = np.empty(GSTR)
    for g in range(NG):
        b[256 * g:256 * (g + 1)] = to_kernel(G6[g])
    b[NG * 256] = spare; b[NG * 256 + 1] = abort
    return b


def pad16(M):
    out = np.zeros((16, 16)); s = M.shape[0]; out[:s, :s] = M
    return out


# ---- consistent inputs ----------------------------------------------------------------------------------------------------------------------
def consistent_gram(s, kappa, seed, n=64):
    """True joint Gram matrices of P, T = A P, R (n x s; P orthonormalised, A SPD with the geometric spectrum 1 ... 1 / kappa), formed in long double
    (64-bit mantissa: consistent far below the fp64 rounding that follows) and rounded to fp64; zero outside s x s.  Returns the six 16 x 16 matrices."""
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((n, n)))[0].astype(LD)
    lam = np.logspace(0.0, -math.log10(kappa), n).astype(LD)
    P = np.linalg.qr(rng.standard_normal((n, s)))[0].astype(LD)
    R = rng.standard_normal((n, s)).astype(LD)
    T = Q @ (lam[:, None] * (Q.T @ P))
    pairs = ((P, T), (P, R), (T, R), (T, T), (R, R), (P, P))
    return [pad16((X.T @ Z).astype(np.float64)) for X, Z in pairs]


# ---- mpmath helpers ---------------------------------------------------------------------------------------------------------------------------
def _m(A):
    return mp.matrix(np.asarray(A, dtype=np.float64).tolist())


def _abs(M):
    return M.apply(abs)


def _sym(M):
    return (M + M.T) / 2


def _np(M):
    return np.array([[float(M[i, j]) for j in range(M.cols)] for i in range(M.rows)])


def exact_algebra(s, G6):
    """c, beta, Grn, Gg of the kernel's comment in exact arithmetic from the inputs alone (mp matrices), and the two condition numbers of the input
    condition: cond(sym P'T), cond(Gg) (2-norm, from the fp64 roundings)."""
    PT, PR, TR, TT, RR, PP = [_m(G[:s, :s]) for G in G6]
    Tm = _sym(PT); Ti = Tm ** -1
    c = -(Ti * PR); V = TT * c + TR; beta = Ti * V
    Grn = _sym(RR + c.T * V + TR.T * c); Gprn = PR + Tm * c
    Gg = Grn - beta.T * Gprn - Gprn.T * beta + beta.T * _sym(PP) * beta
    return dict(c=c, beta=beta, Grn=Grn, Gg=_sym(Gg), cond_T=float(np.linalg.cond(_np(Tm))), cond_G=float(np.linalg.cond(_np(_sym(Gg)))))


def identities(s, G6, mats, rr):
    """The identities (i) ... (v) for outputs mats [4][16][16] and rr of k_xtb_small on the inputs G6.  Returns name -> (|residual|, B, c) as float arrays
    (residual and B rounded from 50 digits; the comparison itself is made in ok())."""
    PT, PR, TR, TT, RR, PP = [_m(G[:s, :s]) for G in G6]
    c, W, M2, M3 = _m(mats[0][:s, :s]), -_m(mats[1][:s, :s]), _m(mats[2][:s, :s]), _m(mats[3][:s, :s])
    Tm = _sym(PT); L = mp.cholesky(Tm); AL = _abs(L) * _abs(L.T); Ti = Tm ** -1
    aW, ac = _abs(W), _abs(c)
    out = {}
    out["i"] = (Tm * c + PR, AL * ac, C1)
    V = TT * c + TR; BV = _abs(TT) * ac + _abs(TR)
    beta = Ti * V; ab = _abs(beta)
    B2 = BV * aW + AL * ab * aW
    out["ii"] = (Tm * M2 - V * W, B2, C2)
    out["iii"] = (M3 + c * W, ac * aW, C3)
    r4 = mp.matrix(1, 1); r4[0, 0] = mp.mpf(float(rr)) - (RR + c.T * V + TR.T * c)[0, 0]
    B_grn = _abs(RR) + ac.T * BV + _abs(TR.T) * ac
    b4 = mp.matrix(1, 1); b4[0, 0] = B_grn[0, 0]
    out["iv"] = (r4, b4, C4)
    PPs = _sym(PP)
    Grn = _sym(RR + c.T * V + TR.T * c); Gprn = PR + Tm * c
    Gg = _sym(Grn - beta.T * Gprn - Gprn.T * beta + beta.T * PPs * beta)
    B_gprn = _abs(PR) + _abs(Tm) * ac
    B_gg = _sym(B_grn) + ab.T * B_gprn + B_gprn.T * ab + ab.T * _abs(PPs) * ab
    Lg = mp.cholesky(Gg)
    B5 = aW.T * (_abs(Lg) * _abs(Lg.T) + B_gg) * aW
    PDW = (PPs * beta - Gprn) * W
    E = (_abs(Ti) * B2 * (C2 // 2)).T * _abs(PDW); E = E + E.T
    rho = max(float(E[i, j] / B5[i, j]) for i in range(s) for j in range(s))
    out["v"] = (W.T * Gg * W - mp.eye(s), B5, CW + int(math.ceil(rho)))
    return {k: (np.abs(_np(r)), _np(B), cc) for k, (r, B, cc) in out.items()}


def w_identity(s, G, W):
    """W' G W - I for a W = Lg^-T the kernel formed from a G it did not have to compute (the set-up pass: G = sym(R'R), one rounding, |G| <= |Lg||Lg'|):
    1 + 17 (factorisation) + 32 (back-substitutions, see CW) = 50, doubled: c = 100, B = |W'||Lg||Lg'||W|."""
    Gm, Wm = _sym(_m(np.asarray(G)[:s, :s])), _m(np.asarray(W)[:s, :s])
    Lg = mp.cholesky(Gm)
    r = Wm.T * Gm * Wm - mp.eye(s)
    B = _abs(Wm.T) * _abs(Lg) * _abs(Lg.T) * _abs(Wm)
    return np.abs(_np(r)), _np(B), 100


def ok(resid, B, c):
    """|residual| <= c u B element by element (NaN fails); the count must keep c u <= 1e-12"""
    assert c * U <= 1e-12, c
    return bool(np.all(resid <= c * U * B))


def ratio(resid, B):
    """largest |residual| / (u B) (what the tests print)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(B > 0, resid / (U * B), np.where(resid == 0, 0.0, np.inf))
    return float(np.max(q))


def shape_ok(s, mats):
    """W upper triangular; c, W, M2, M3 zero outside s x s"""
    W = -np.asarray(mats[1])
    outside = np.ones((16, 16), dtype=bool); outside[:s, :s] = False
    return bool(np.all(np.tril(W, -1) == 0.0)) and all(bool(np.all(np.asarray(mats[k])[outside] == 0.0)) for k in range(4))


# ---- a numpy fp64 restatement of k_xtb_small (CPU validation of this reference; NOT bit-identical to the kernel) ----------------------------------
def new_ctrl(**kw):
    c = dict(rr=[0.0, 0.0], done_local=0, sharded=0, done=0, iters=0, abort_local=0, aborted=0, pad=[0, 0], xchg_timeout=0, pad2=0)
    c.update(kw)
    return c


def _chol(A, s):
    """lower Cholesky factor of the leading s x s block as the kernel forms it: a non-positive pivot is replaced by 1 and reported"""
    Lf = np.array(A[:s, :s]); good = True
    for k in range(s):
        d = Lf[k, k]
        if not d > 0.0:
            good = False
        ld = math.sqrt(d if d > 0.0 else 1.0)
        Lf[k, k] = ld
        Lf[k + 1:, k] /= ld
        for j in range(k + 1, s):
            Lf[j:, j] -= Lf[j:, k] * Lf[j, k]
    return np.tril(Lf), good


def _chol_solve(Lf, B):
    from scipy.linalg import solve_triangular
    return solve_triangular(Lf.T, solve_triangular(Lf, B, lower=True), lower=False)


def small_fp64(it, s, blocks, tol2, ctrl, mats):
    """blocks: list (one per rank) of (G6, abort word); ctrl: new_ctrl(...); mats [4][16][16]: the pre-fill.  Returns (mats, ctrl) afterwards."""
    ctrl = {k: (list(v) if isinstance(v, list) else v) for k, v in ctrl.items()}
    mats = np.array(mats, dtype=np.float64)
    if ctrl["done"]:
        return mats, ctrl
    if len(blocks) > 1 and any(a != 0.0 for _, a in blocks):
        ctrl["aborted"] = 1; ctrl["done"] = max(it + 1, 1)
        return mats, ctrl
    G = [np.array(blocks[0][0][g], dtype=np.float64) for g in range(NG)]
    for G6, _ in blocks[1:]:
        for g in range(NG):
            G[g] = G[g] + G6[g]
    G = [X[:s, :s] for X in G]
    sym = lambda X: 0.5 * (X + X.T)
    if it < 0:
        c = np.zeros((s, s)); beta = np.zeros((s, s)); Grn = sym(G[4]); Gg = Grn.copy()
    else:
        Tm = sym(G[0])
        Lp, good = _chol(Tm, s)
        if not good:
            ctrl["pad"][0] = 1; ctrl["done"] = it + 1
            return mats, ctrl
        c = -_chol_solve(Lp, G[1])
        V = G[3] @ c + G[2]
        beta = _chol_solve(Lp, V)
        Grn = sym((G[2].T @ c) + ((c.T @ V) + G[4]))
        Gprn = Tm @ c + G[1]
        Gg = sym(G[5]) @ beta
        Gg = beta.T @ Gg + Grn
        Gg = -(beta.T @ Gprn) + Gg
        Gg = sym(-(Gprn.T @ beta) + Gg)
    rr = Grn[0, 0]
    stop = (not math.sqrt(rr) > tol2) if it < 0 else (not rr > tol2)      # (rr < 0: sqrt gives NaN on the device; not reached by the tests)
    diag_ok = bool(np.all(np.diag(Gg) > 0.0))
    Lg, cholg = _chol(Gg, s)
    if not cholg:
        Lg = np.diag(np.sqrt(np.where(diag_ok, np.diag(Gg), 1.0)))
    from scipy.linalg import solve_triangular
    W = solve_triangular(Lg.T, np.eye(s), lower=False) if diag_ok else np.zeros((s, s))
    mats[0] = pad16(c); mats[1] = pad16(-W); mats[2] = pad16(beta @ W); mats[3] = pad16(-(c @ W))
    ctrl["rr"] = [rr, rr]; ctrl["iters"] = it + 1
    if not diag_ok:
        ctrl["pad"][0] = 2
    elif not cholg:
        ctrl["pad"][1] += 1
    if stop or not diag_ok:
        if ctrl["sharded"]:
            ctrl["done_local"] = 1
        else:
            ctrl["done"] = it + 2
    return mats, ctrl


# ---- crafted inputs of the decision and breakdown branches --------------------------------------------------------------------------------------
def branch_inputs(s, RR, PT=None, junk=False, seed=0):
    """P'R = T'R = 0, so c = beta = 0 exactly and the direction Gram matrix IS sym(R'R) = RR (s x s, symmetric).  P'T: the identity unless given;
    T'T, P'P: identities, or -- junk -- arbitrary dense matrices (they meet only zeros)."""
    rng = np.random.default_rng(seed)
    Z = np.zeros((s, s)); I = np.eye(s)
    TT, PP = (rng.standard_normal((s, s)), rng.standard_normal((s, s))) if junk else (I, I)
    return [pad16(X) for X in (I if PT is None else PT, Z, Z, TT, np.asarray(RR, dtype=np.float64), PP)]


def indefinite_rr(s):
    """symmetric, positive diagonal, not positive definite (s >= 2): the 2 x 2 block [[1, 2], [2, 1]] in front of a diagonal 4, 9, 16 ..."""
    RR = np.diag(np.arange(1, s + 1, dtype=np.float64) ** 2)
    RR[0, 0] = RR[1, 1] = 1.0; RR[0, 1] = RR[1, 0] = 2.0
    return RR
