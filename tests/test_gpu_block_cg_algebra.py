"""The last four launches of a preconditioned block-CG sweep (csrc/xtb.hip: k_xtb_rows<0, 0, 1>, k_xtb_gred, k_xtb_small, k_xtb_step) against plain
high-precision references of the same operations.  Whole solves only assert a final true residual and a sweep count, and the loop corrects itself: a
wrong beta, a row counted twice in a Gram matrix or a wrong breakdown decision costs sweeps at most.  These tests run the production kernels on
caller-given data (dkmc_xtb_test_gram / _small / _step) and compare what they wrote.

Method (tests/test_gpu_precond_reference.py): element by element |gpu - ref| <= c u B, u = 2^-53, B the same expression with every term in absolute
value, c a count of roundings derived next to the assertion (c u <= 1e-12 is asserted by the helpers); exact or bitwise where the arithmetic is exact.
Sums and products: numpy.longdouble; the s x s algebra: mpmath at 50 digits (tests/block_cg_algebra_ref.py, which also derives the counts of b).
Every group carries a negative control that the same assertion rejects.

a. Gram matrices: integer panels bitwise against an integer reference, real-valued panels with rows scaled over 1e-6 ... 1e6 within the count of the
   kernel's grouping; row counts around the 4-row k-step, the 16- and 64-row wave steps and above 131 072, 1 ... 4096 workgroups (most of them with an
   empty chunk at the small sizes), no / all / a shuffled half of the rows as S rows.
b. The s x s algebra on consistent Gram matrices: identities (i) - (v) of the reference, from the inputs and the kernel's own outputs.
c. The stop test and every breakdown branch on crafted inputs (c = beta = 0 exactly): exact values of XCtrl and mats.
d. The panel step against the long-double reference formed from the ORIGINAL panels; QS bitwise; row lists; the iteration-stamped stop word.

Every comparison within c u B prints the largest multiple of u B it met (-s); the docstrings quote those of an MI355X."""
import ctypes as C

import numpy as np
import pytest

import block_cg_algebra_ref as ref
from devicekmc_amd import lib as dlib
from devicekmc_amd.lib import check
from test_gpu_parity import Vd, hip  # noqa: F401

pytestmark = pytest.mark.gpu

U = ref.U
LD = np.longdouble


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _ok(gpu, ref_, B, c):
    """Element-wise |gpu - ref| <= c u B (NaN fails)."""
    assert np.all(c * U <= 1e-12)
    return np.abs(gpu.astype(LD) - ref_) <= LD(c * U) * B


def _worst(gpu, ref_, B):
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(B > 0, np.abs(gpu.astype(LD) - ref_) / (LD(U) * B), 0)
    return float(np.max(q))


def _ctrl_dict(c):
    return dict(rr=list(c.rr), done_local=c.done_local, sharded=c.sharded, done=c.done, iters=c.iters, abort_local=c.abort_local, aborted=c.aborted,
                pad=list(c.pad), xchg_timeout=c.xchg_timeout, pad2=c.pad2)


def _ctrl_struct(d):
    c = dlib.dkmc_xtb_ctrl()
    for k, v in d.items():
        if isinstance(v, list):
            for i, x in enumerate(v):
                getattr(c, k)[i] = x
        else:
            setattr(c, k, v)
    return c


# ---- a. Gram matrices ------------------------------------------------------------------------------------------------------------------------
GRAM_M = [2, 3, 5, 17, 63, 64, 65, 257, 4099, 200003]
GRAM_NG = [1, 7, 128, 4096]
PAIRS = ((0, 1), (0, 2), (1, 2), (1, 1), (2, 2), (0, 0))                 # (P, T, R) = panels 0, 1, 2: P'T, P'R, T'R, T'T, R'R, P'P


def _sranks(m, kind, rng):
    """nsrank[m], ns: no S row, all rows (in a random order), or a shuffled random half with rows 0 and 1 in it whose count is no multiple of 32"""
    nsrank = np.full(m, -1, dtype=np.int32)
    if kind == "none":
        return nsrank, 0
    if kind == "all":
        rows = np.arange(m)
    else:
        rows = np.union1d(np.flatnonzero(rng.random(m) < 0.5), [0, 1])
        if len(rows) % 32 == 0:
            rest = np.setdiff1d(np.arange(m), rows)
            rows = np.append(rows, rest[0]) if len(rest) else rows[:-1]
        assert len(rows) % 32 != 0 and 0 in rows and 1 in rows
    rows = rng.permutation(rows)
    nsrank[rows] = np.arange(len(rows), dtype=np.int32)
    return nsrank, len(rows)


def _gram(L, panels, nsrank, ns, ng, done=0, prefill=None):
    gfin = np.full(6 * 256, np.nan) if prefill is None else prefill.copy()
    ctrl = dlib.dkmc_xtb_ctrl()
    check(L.dkmc_xtb_test_gram(panels[0].shape[0], _p(panels[0]), _p(panels[1]), _p(panels[2]), _p(nsrank), ns, ng, done, _p(gfin), C.byref(ctrl)))
    return gfin, ctrl


def _natural(gfin):
    return np.stack([ref.from_kernel(gfin[256 * g:256 * (g + 1)]) for g in range(6)])


@pytest.mark.parametrize("m", GRAM_M)
def test_gram_integer_panels_are_exact(hip, m):
    """Entries in [-8, 8]: every Gram entry is an integer below 2^53 however the additions are grouped, so the six matrices equal the integer reference
    exactly -- a row counted twice or never (S rows take another path than the others), a wrong pair of operands or a transposed matrix cannot pass."""
    host, L = hip
    rng = np.random.default_rng(1000 + m)
    kinds = {k: _sranks(m, k, rng) for k in ("none", "all", "half")}
    runs = 0
    for s in (1, 3, 16):
        pan = [np.zeros((m, 16)) for _ in range(3)]
        ipan = [rng.integers(-8, 9, (m, s)) for _ in range(3)]
        for a, b in zip(pan, ipan):
            a[:, :s] = b
        want = np.zeros((6, 16, 16))
        for g, (x, z) in enumerate(PAIRS):
            want[g, :s, :s] = ipan[x].T @ ipan[z]                         # int64: exact
        assert np.abs(want).max() < 2.0 ** 53
        for ng in GRAM_NG:
            for kind, (nsrank, ns) in kinds.items():
                gfin, ctrl = _gram(L, pan, nsrank, ns, ng)
                got = _natural(gfin)
                assert np.array_equal(got, want), (m, s, ng, kind, np.argwhere(got != want)[:4])
                assert _ctrl_dict(ctrl) == ref.new_ctrl(), (m, s, ng, kind)
                runs += 1
        # negative control: the reference with row 0 counted twice is another matrix wherever that row is not zero
        twice = want.copy()
        for g, (x, z) in enumerate(PAIRS):
            twice[g, :s, :s] += np.outer(ipan[x][0], ipan[z][0])
        if np.any(twice != want):
            assert not np.array_equal(got, twice)
    assert runs == 3 * len(GRAM_NG) * 3


def _gram_count(m, ns, ng):
    """Roundings behind one entry.  A wave adds its rows in ONE chain of fused multiply-adds (v_mfma_f64_16x16x4: four rows per instruction): per 64-row
    round of its workgroup's chunk 16 rows, and 8 rows of each S block of 32 -- with the rows that are masked out counted as terms.  Then the four waves in
    two levels (2), k_xtb_gred's slice of ceil(ng / 16) partials in four chains and two levels (ceil(ng / 64) + 2), and the 16 slices in order (16)."""
    chunk = (-(-m // ng) + 3) & ~3
    nK = -(-ns // 32)
    wave = 16 * -(-chunk // 64) + 8 * -(-nK // ng)
    return wave + 2 + -(-ng // 64) + 2 + 16 + 1                            # (+ 1: the reference's own error, _ld_gram)


def _ld_gram(X, Z, chunk=512):
    """X'Z in long double, added chunk by chunk: the reference's own error is (chunk + m / chunk) 2^-64 B at the most, below u B / 2 for m <= 2e5"""
    acc = np.zeros((16, 16), dtype=LD)
    for i in range(0, X.shape[0], chunk):
        acc += X[i:i + chunk].T @ Z[i:i + chunk]
    return acc


@pytest.mark.parametrize("m", GRAM_M)
def test_gram_real_valued_panels(hip, m):
    """Standard normal entries, rows scaled by 10^uniform(-6, 6) (the scale of a row is shared by the three panels, as a residual's rows are), against
    the long-double reference within the count of _gram_count.  Negative control: the reference without the row of the largest scale.
    Measured on an MI355X, largest |gpu - ref| / (u B) over the twelve runs of a size: 1.0 (m = 2), 1.7, 2.5, 3.7, 5.5, 4.6, 5.2, 4.6 (m = 257), 13.7
    (m = 4099) and 38.8 (m = 200003), against counts of 38 (one workgroup at the smallest sizes) ... 2094 (m = 4099, all rows S rows, one workgroup).  The run closest to its own count: 5.51 u B of 47
    (m = 63); at m = 200003 3.06 of 101 (ng = 4096)."""
    host, L = hip
    rng = np.random.default_rng(2000 + m)
    scale = 10.0 ** rng.uniform(-6, 6, (m, 1))
    scale[rng.integers(0, m)] = 1e6; scale[rng.integers(0, m)] = 1e-6
    pan = [np.ascontiguousarray(rng.standard_normal((m, 16)) * scale) for _ in range(3)]
    lp = [p.astype(LD) for p in pan]
    want = np.stack([_ld_gram(lp[x], lp[z]) for x, z in PAIRS])
    B = np.stack([(np.abs(pan[x]).T @ np.abs(pan[z])).astype(LD) for x, z in PAIRS]) * LD(1 + 1e-9)      # (fp64: B is a bound, 1e-9 covers its rounding)
    drop = int(np.argmax(scale))
    without = want - np.stack([np.outer(lp[x][drop], lp[z][drop]) for x, z in PAIRS])
    worst, runs = (0.0, 1), 0
    for kind in ("none", "all", "half"):
        nsrank, ns = _sranks(m, kind, rng)
        for ng in GRAM_NG:
            c = _gram_count(m, ns, ng)
            if c * U > 1e-12:
                assert m > 131072 and ng < 128                           # one or seven workgroups for 2e5 rows: chains no count of 1e-12 / u covers
                continue
            gfin, _ = _gram(L, pan, nsrank, ns, ng)
            got = _natural(gfin)
            good = _ok(got, want, B, c)
            worst = max(worst, (_worst(got, want, B), c), key=lambda t: t[0] / t[1])
            assert good.all(), (m, kind, ng, c, np.argwhere(~good)[:4], _worst(got, want, B))
            assert not _ok(got, without, B, c).all(), (m, kind, ng)
            runs += 1
    print("gram m = %d: closest to its count: |gpu - ref| = %.2f u B of %d" % ((m,) + worst))
    assert runs == 12 if m < 131072 else runs >= 6


def test_gram_preset_stop_word_and_bad_arguments(hip):
    host, L = hip
    rng = np.random.default_rng(3)
    m = 65
    pan = [rng.standard_normal((m, 16)) for _ in range(3)]
    nsrank, ns = _sranks(m, "half", rng)
    pre = rng.standard_normal(6 * 256)
    gfin, ctrl = _gram(L, pan, nsrank, ns, 7, done=3, prefill=pre)
    assert gfin.tobytes() == pre.tobytes() and _ctrl_dict(ctrl) == ref.new_ctrl(done=3)
    gfin, _ = _gram(L, pan, nsrank, ns, 7, done=0, prefill=pre)
    assert not np.any(gfin == pre)
    dup = nsrank.copy(); dup[np.flatnonzero(nsrank < 0)[0]] = 0            # a rank twice
    hole = nsrank.copy(); hole[nsrank == 0] = -1                           # a rank never
    ct = dlib.dkmc_xtb_ctrl()
    for args in ((m, _p(pan[0]), _p(pan[1]), _p(pan[2]), _p(dup), ns, 7), (m, _p(pan[0]), _p(pan[1]), _p(pan[2]), _p(hole), ns, 7),
                 (m, _p(pan[0]), _p(pan[1]), _p(pan[2]), _p(nsrank), ns, 0), (m, _p(pan[0]), _p(pan[1]), _p(pan[2]), _p(nsrank), ns, 4097),
                 (0, _p(pan[0]), _p(pan[1]), _p(pan[2]), _p(nsrank), ns, 7), (m, None, _p(pan[1]), _p(pan[2]), _p(nsrank), ns, 7),
                 (m, _p(pan[0]), _p(pan[1]), _p(pan[2]), _p(nsrank), ns + 1, 7)):
        assert L.dkmc_xtb_test_gram(*args, 0, _p(pre), C.byref(ct)) != 0, args[5:]
        L.dkmc_clear_error()


# ---- b. / c. the s x s algebra ------------------------------------------------------------------------------------------------------------------
PRE = np.arange(4 * 256, dtype=np.float64).reshape(4, 16, 16) / 8 + 0.375      # the pre-fill of mats: no value the algebra would write


def _small(L, it, s, blocks, tol2, ctrl=None, mats=PRE):
    """blocks: list of (G6, abort word).  Returns mats [4][16][16] and the XCtrl (dict) afterwards."""
    gb = np.concatenate([ref.gram_block(G6, abort=a) for G6, a in blocks])
    out = np.ascontiguousarray(mats, dtype=np.float64).copy()
    cin = _ctrl_struct(ctrl or ref.new_ctrl()); cout = dlib.dkmc_xtb_ctrl()
    check(L.dkmc_xtb_test_small(it, s, len(blocks), _p(gb), tol2, C.byref(cin), _p(out), C.byref(cout)))
    return out, _ctrl_dict(cout)


@pytest.mark.parametrize("s", [1, 2, 3, 8, 15, 16])
def test_small_identities_on_consistent_inputs(hip, s):
    """True joint Gram matrices of P (orthonormalised), T = A P, R with n = 64 and kappa(A) = 1e2, 1e4, 1e6, zero outside s x s -- the contract xtb_mm
    states, and what production feeds it: the loop keeps columns >= s of P, T, R zero (k_xtb_init and xtb_rhs write zeros there, every later panel
    is a product with a matrix that is zero outside s x s), so k_xtb_rows sums zeros.  Input condition, checked by the reference: cond(sym P'T) and cond of
    the exact direction Gram matrix <= 1e6 (here at most 1.4e2 and 6e3), and the count of (v) within 1e-12 / u.
    Identities (tests/block_cg_algebra_ref.py, mpmath, from the inputs and the outputs under test):
      (i) Tm c + P'R; (ii) Tm M2 - V W; (iii) M3 + c W; (iv) rr; (v) W upper triangular, zero outside s x s, W' Gg W - I.
    Negative controls: the largest entry of P'R changed by 1e-9 of itself (rejected by (i)), M3 with the wrong sign (rejected by (iii)).
    Measured on an MI355X, largest multiples of u B over the 18 inputs (counts): (i) 3.00 (100), (ii) 1.16 (170), (iii) 1.54 (17), (iv) 0.63 (54),
    (v) 3.38 (233 ... 5500, the count growing with cond(sym P'T): see the reference's header)."""
    host, L = hip
    it = 3
    for kappa in (1e2, 1e4, 1e6):
        G6 = ref.consistent_gram(s, kappa, seed=400000 + 1000 * s + int(round(np.log10(kappa))))
        ex = ref.exact_algebra(s, G6)
        assert ex["cond_T"] <= 1e6 and ex["cond_G"] <= 1e6
        mats, ctrl = _small(L, it, s, [(G6, 0.0)], 1e-300)
        assert ref.shape_ok(s, mats), (s, kappa)
        assert ctrl["rr"][0] == ctrl["rr"][1]
        assert ctrl == ref.new_ctrl(rr=ctrl["rr"], iters=it + 1), (s, kappa, ctrl)       # iters = it + 1; done, done_local, pad and the rest: 0
        ids = ref.identities(s, G6, mats, ctrl["rr"][0])
        print("small s = %d kappa = %.0e:" % (s, kappa), " ".join("(%s) %.2f of %d" % (n, ref.ratio(r, B), c) for n, (r, B, c) in ids.items()))
        for name, (r, B, c) in ids.items():
            assert ref.ok(r, B, c), (s, kappa, name, ref.ratio(r, B), c)
        G6b = [G.copy() for G in G6]
        k = np.unravel_index(np.argmax(np.abs(G6b[1])), (16, 16)); G6b[1][k] *= 1 + 1e-9
        r, B, c = ref.identities(s, G6b, mats, ctrl["rr"][0])["i"]
        assert not ref.ok(r, B, c), (s, kappa)
        bad = mats.copy(); bad[3] = -bad[3]
        r, B, c = ref.identities(s, G6, bad, ctrl["rr"][0])["iii"]
        assert not ref.ok(r, B, c), (s, kappa)


def _wdiag_ok(mats, s, g):
    """W = diag(1 / sqrt(g_ii)) within 2 u (one square root, one division), zero elsewhere"""
    W = -mats[1]
    d = np.diag(W)[:s].astype(LD); want = 1 / np.sqrt(np.asarray(g, dtype=LD))
    return np.array_equal(W, np.diag(np.diag(W))) and not np.diag(W)[s:].any() and bool(np.all(np.abs(d - want) <= 2 * LD(U) * want))


@pytest.mark.parametrize("s", [3, 16])
def test_small_stop_decisions(hip, s):
    """rr a factor 4 on either side of the stop test: rr against tol2 for it >= 0, sqrt(rr) for the set-up pass (tol2 and rr chosen so that the other
    reading of the test decides the other way).  c = beta = 0 exactly, the direction Gram matrix is diag(R'R).  Negative control: the outcomes of the
    two sides differ, so an assertion on one rejects the other."""
    host, L = hip
    diag = lambda rr: np.concatenate([[rr], np.arange(5.0, 4.0 + s)])
    for it, tol2, above, below in ((2, 100.0, 400.0, 25.0), (0, 100.0, 400.0, 25.0), (-1, 0.01, 0.04 ** 2, 0.0025 ** 2)):
        seen = []
        for rr, stops in ((above, False), (below, True)):
            G6 = ref.branch_inputs(s, np.diag(diag(rr)))
            for sharded in (0, 1):
                mats, c = _small(L, it, s, [(G6, 0.0)], tol2, ref.new_ctrl(sharded=sharded))
                want = ref.new_ctrl(rr=[rr, rr], iters=it + 1, sharded=sharded)
                if stops:
                    want["done_local" if sharded else "done"] = 1 if sharded else it + 2
                assert c == want, (s, it, rr, sharded, c)
                assert not mats[0].any() and not mats[2].any() and not mats[3].any()
                assert _wdiag_ok(mats, s, diag(rr)), (s, it, rr)
                seen.append((c["done"], c["done_local"]))
        assert seen == [(0, 0), (0, 0), (it + 2, 0), (0, 1)]


@pytest.mark.parametrize("s", [2, 3, 16])
def test_small_breakdown_branches(hip, s):
    """Exact values of XCtrl and mats in every breakdown branch (it = 4; pad[1] preset to 5)."""
    host, L = hip
    it, start = 4, ref.new_ctrl(pad=[0, 5])
    good_rr = np.diag(np.arange(4.0, 4.0 + s))
    # lost definiteness with a positive diagonal: pad[1] counts it, W only rescales, the loop goes on
    RR = ref.indefinite_rr(s)
    mats, c = _small(L, it, s, [(ref.branch_inputs(s, RR), 0.0)], 1e-300, start)
    assert c == ref.new_ctrl(rr=[1.0, 1.0], iters=it + 1, pad=[0, 6]), c
    assert _wdiag_ok(mats, s, np.diag(RR)) and not mats[0].any() and not mats[2].any() and not mats[3].any()
    # (negative control: a definite matrix of the same diagonal takes the other branch)
    mats, c = _small(L, it, s, [(ref.branch_inputs(s, np.diag(np.diag(RR))), 0.0)], 1e-300, start)
    assert c["pad"] == [0, 5]
    # a zero / a negative diagonal entry: pad[0] = 2, W = M2 = M3 = 0, the loop ends behind this iteration's step
    for d in (0.0, -1.0):
        bad = good_rr.copy(); bad[s - 1, s - 1] = d
        mats, c = _small(L, it, s, [(ref.branch_inputs(s, bad), 0.0)], 1e-300, start)
        assert c == ref.new_ctrl(rr=[4.0, 4.0], iters=it + 1, pad=[2, 5], done=it + 2), (s, d, c)
        assert not mats.any(), (s, d)
        mats, c = _small(L, it, s, [(ref.branch_inputs(s, bad), 0.0)], 1e-300, ref.new_ctrl(pad=[0, 5], sharded=1))
        assert c == ref.new_ctrl(rr=[4.0, 4.0], iters=it + 1, pad=[2, 5], done_local=1, sharded=1), (s, d, c)
    # P'T with a non-positive first / later pivot: pad[0] = 1, stop BEFORE this iteration's step, nothing else written
    first = np.eye(s); first[0, 0] = -1.0
    zero = np.eye(s); zero[0, 0] = 0.0
    later = np.eye(s); later[s - 2:, s - 2:] = [[1.0, 2.0], [2.0, 1.0]]
    for PT in (first, zero, later):
        mats, c = _small(L, it, s, [(ref.branch_inputs(s, good_rr, PT=PT), 0.0)], 1e-300, start)
        assert c == ref.new_ctrl(pad=[1, 5], done=it + 1), (s, c)
        assert mats.tobytes() == PRE.tobytes(), s
    # (negative control: the identity for P'T runs through)
    mats, c = _small(L, it, s, [(ref.branch_inputs(s, good_rr), 0.0)], 1e-300, start)
    assert c == ref.new_ctrl(rr=[4.0, 4.0], iters=it + 1, pad=[0, 5]) and mats.tobytes() != PRE.tobytes()
    # a preset stop word: nothing is written
    for done in (1, it + 1, it + 2, 99):
        cin = ref.new_ctrl(done=done, pad=[0, 5], rr=[3.0, 2.0], iters=2)
        mats, c = _small(L, it, s, [(ref.branch_inputs(s, good_rr), 0.0)], 1e-300, cin)
        assert c == cin and mats.tobytes() == PRE.tobytes(), (s, done)


@pytest.mark.parametrize("s", [1, 3, 16])
def test_small_setup_pass_reads_only_rr(hip, s):
    """it = -1: c = M2 = M3 = 0 and W from sym(R'R) alone, whatever the other five matrices hold (dense junk, outside s x s too); R'R itself is given
    unsymmetric.  W' sym(R'R) W - I within 100 u |W'||Lg||Lg'||W| (ref.w_identity).  Negative control: W scaled by 1 + 1e-9.
    Measured on an MI355X: 2.16, 1.21 and 2.06 u B (s = 1, 3, 16) of 100."""
    host, L = hip
    rng = np.random.default_rng(40 + s)
    X = rng.standard_normal((40, s))
    RR = X.T @ X + 1e-3 * np.triu(rng.standard_normal((s, s)), 1)
    G6 = [rng.standard_normal((16, 16)) for _ in range(6)]
    G6[4] = ref.pad16(RR)
    mats, c = _small(L, -1, s, [(G6, 0.0)], 1e-300)
    rr = 0.5 * (RR[0, 0] + RR[0, 0])
    assert c == ref.new_ctrl(rr=[rr, rr], iters=0), c
    assert not mats[0].any() and not mats[2].any() and not mats[3].any() and ref.shape_ok(s, mats)
    r, B, cnt = ref.w_identity(s, RR, -mats[1])
    print("set-up pass s = %d: W' G W - I at %.2f u B of %d" % (s, ref.ratio(r, B), cnt))
    assert ref.ok(r, B, cnt)
    r, B, cnt = ref.w_identity(s, RR, -mats[1] * (1 + 1e-9))
    assert not ref.ok(r, B, cnt)
    # the same bits with the other five matrices zero
    clean = [np.zeros((16, 16)) for _ in range(6)]; clean[4] = G6[4]
    mats2, c2 = _small(L, -1, s, [(clean, 0.0)], 1e-300)
    assert mats2.tobytes() == mats.tobytes() and c2 == c


@pytest.mark.parametrize("nrg", [1, 2, 4, 5, 8, 9])
def test_small_adds_the_ranks_blocks_in_rank_order(hip, nrg):
    """nrg blocks (batches of four and every tail length): the same bits as ONE block holding the blocks added in rank order with plain sequential fp64
    additions on the host.  With one rank's abort word set: aborted = 1, done = max(it + 1, 1), mats untouched.  Negative control: the blocks added in
    the reverse order give other bits."""
    host, L = hip
    s, it = 16, 3
    rng = np.random.default_rng(70 + nrg)
    G6 = ref.consistent_gram(s, 1e4, seed=77)
    w = rng.uniform(0.5, 1.5, nrg); w /= w.sum()
    parts = [[w[r] * G + 1e-6 * w[r] * np.abs(G).max() * rng.standard_normal((16, 16)) for G in G6] for r in range(nrg)]
    def added(order):
        tot = [parts[order[0]][g].copy() for g in range(6)]
        for r in order[1:]:
            for g in range(6):
                tot[g] = tot[g] + parts[r][g]
        return tot
    many, cm = _small(L, it, s, [(p, 0.0) for p in parts], 1e-300)
    one, c1 = _small(L, it, s, [(added(list(range(nrg))), 0.0)], 1e-300)
    assert cm["pad"] == [0, 0] and cm["done"] == 0 and cm["iters"] == it + 1 and many.tobytes() != PRE.tobytes()
    assert many.tobytes() == one.tobytes() and cm == c1, nrg
    if nrg > 2:
        rev, _ = _small(L, it, s, [(added(list(range(nrg))[::-1]), 0.0)], 1e-300)
        assert rev.tobytes() != one.tobytes()
    if nrg > 1:
        for it2 in (-1, 0, 3):
            for who in {0, nrg // 2, nrg - 1}:
                mats, c = _small(L, it2, s, [(p, 1.0 if r == who else 0.0) for r, p in enumerate(parts)], 1e-300)
                assert c == ref.new_ctrl(aborted=1, done=max(it2 + 1, 1)), (nrg, it2, who, c)
                assert mats.tobytes() == PRE.tobytes()


def test_small_refuses_bad_arguments(hip):
    host, L = hip
    gb = ref.gram_block(ref.branch_inputs(3, np.eye(3)))
    cin, cout, mats = dlib.dkmc_xtb_ctrl(), dlib.dkmc_xtb_ctrl(), PRE.copy()
    for it, s, nrg in ((-2, 3, 1), (0, 0, 1), (0, 17, 1), (0, 3, 0), (0, 3, 65)):
        assert L.dkmc_xtb_test_small(it, s, nrg, _p(gb), 1.0, C.byref(cin), _p(mats), C.byref(cout)) != 0, (it, s, nrg)
        L.dkmc_clear_error()
    assert L.dkmc_xtb_test_small(0, 3, 1, None, 1.0, C.byref(cin), _p(mats), C.byref(cout)) != 0
    L.dkmc_clear_error()


# ---- d. panel step -----------------------------------------------------------------------------------------------------------------------------
STEP_M = [1, 2, 15, 16, 17, 63, 65, 4099, 140003]


def _step(L, it, mats, done, y0, R, P, T, sc, nsrank, ns, rowlist=None, Y=None, qs=None):
    y0, R, P = y0.copy(), R.copy(), P.copy()
    Y = None if Y is None else Y.copy()
    qs = None if ns == 0 else qs.copy()
    check(L.dkmc_xtb_test_step(len(y0), it, _p(np.ascontiguousarray(mats)), done, _p(y0), _p(R), _p(P), _p(T), _p(sc), _p(nsrank), ns, _p(rowlist),
                               0 if rowlist is None else len(rowlist), _p(Y), _p(qs)))
    return y0, R, P, Y, qs


def _step_mats(s, rng):
    """c | M1 | M2 | M3 random, dense inside s x s and zero outside; M3 is NOT c M1, so the three products of P are told apart"""
    mats = np.zeros((4, 16, 16))
    mats[:, :s, :s] = rng.standard_normal((4, s, s))
    return mats


def _step_reference(mats, y0, R, P, T, Y):
    """long double, from the ORIGINAL panels.  Returns name -> (ref, B, c); B in fp64 with 1e-9 for its own rounding:
    y0 + P c(:, 0): per lane two products and their sum, twice, added (3 roundings deep), two more additions across the lanes, the addition to y0: 6, c = 8
    R + T c, Y + P c: a chain of 16 fused multiply-adds on the input: c = 17
    R M1 + T M3 + P M2: a chain of 48: c = 49"""
    c, M1, M2, M3 = [x.astype(LD) for x in mats]
    a = np.abs(mats)
    lR, lP, lT = R.astype(LD), P.astype(LD), T.astype(LD)
    aR, aP, aT = np.abs(R), np.abs(P), np.abs(T)
    up = LD(1 + 1e-9)
    return {"y0": (y0.astype(LD) + lP @ c[:, 0], (np.abs(y0) + aP @ a[0][:, 0]) * up, 8),
            "R": (lR + lT @ c, (aR + aT @ a[0]) * up, 17),
            "P": (lR @ M1 + lT @ M3 + lP @ M2, (aR @ a[1] + aT @ a[3] + aP @ a[2]) * up, 49),
            "Y": (Y.astype(LD) + lP @ c, (np.abs(Y) + aP @ a[0]) * up, 17)}


@pytest.mark.parametrize("m", STEP_M)
def test_step_against_the_original_panels(hip, m):
    """Y += P c, R += T c, P = R M1 + T M3 + P M2 from the ORIGINAL R, T, P, with and without Ypanel; QS bitwise sc[row] P_out[row] at the S rows; with a
    shuffled row list whose length is no multiple of 16 only the listed rows change (the others hold NaN before and after, their QS rows the pre-fill).
    140003 rows (s = 16 only): the grid-stride loop of the 2048 workgroups runs.  Negative control: P formed with the updated R.
    Measured on an MI355X, largest |gpu - ref| / (u B) over the sizes (counts): y0 2.53 (8), R 5.20 (17), Y 4.93 (17), P 5.69 (49), each at the two
    largest sizes; at 65 rows and below none exceeds 2.8."""
    host, L = hip
    rng = np.random.default_rng(5000 + m)
    it = 6
    y0 = rng.standard_normal(m); sc = rng.uniform(0.5, 2.0, m)
    R, P, T, Y = [rng.standard_normal((m, 16)) for _ in range(4)]
    nsrank, ns = _sranks(m, "half", rng) if m > 1 else (np.zeros(1, dtype=np.int32), 1)
    qs0 = rng.standard_normal((ns, 16)) + 100.0
    srows = np.flatnonzero(nsrank >= 0)
    worst = {}
    for s in ((3, 16) if m < 100000 else (16,)):
        mats = _step_mats(s, rng)
        want = _step_reference(mats, y0, R, P, T, Y)
        for Yp in (None, Y):
            y1, R1, P1, Y1, qs1 = _step(L, it, mats, 0, y0, R, P, T, sc, nsrank, ns, Y=Yp, qs=qs0)
            got = {"y0": y1, "R": R1, "P": P1, "Y": Y1}
            for name, (rf, B, c) in want.items():
                if got[name] is None:
                    continue
                good = _ok(got[name], rf, B, c)
                worst[name] = max(worst.get(name, 0.0), _worst(got[name], rf, B))
                assert good.all(), (m, s, name, np.argwhere(~good)[:4], _worst(got[name], rf, B))
            if s < 16:
                assert R1[:, s:].tobytes() == R[:, s:].tobytes() and not P1[:, s:].any()      # columns >= s: R as it was, P zero
            assert np.array_equal(qs1[nsrank[srows]], sc[srows, None] * P1[srows]), (m, s)
        # negative control: the reference of P formed with the updated R in place of the original one is rejected
        rf, B, c = want["P"]
        assert not _ok(P1, rf + (R1.astype(LD) - R.astype(LD)) @ mats[1].astype(LD), B, c).all(), (m, s)
        # row list
        if m >= 2:
            lst = np.union1d(np.flatnonzero(rng.random(m) < 0.6), [0, 1])
            if len(lst) == m and m > 2:
                lst = lst[lst != 2]
            if len(lst) % 16 == 0:
                lst = lst[:-1]
            rowlist = rng.permutation(lst).astype(np.int32)
            assert len(rowlist) % 16 != 0
            listed = np.zeros(m, dtype=bool); listed[rowlist] = True
            yn, Rn, Pn, Tn, Yn = y0.copy(), R.copy(), P.copy(), T.copy(), Y.copy()
            for a in (yn, Rn, Pn, Tn, Yn):
                a[~listed] = np.nan
            y1, R1, P1, Y1, qs1 = _step(L, it, mats, 0, yn, Rn, Pn, Tn, sc, nsrank, ns, rowlist=rowlist, Y=Yn, qs=qs0)
            got = {"y0": y1, "R": R1, "P": P1, "Y": Y1}
            for name, (rf, B, c) in want.items():                             # (row by row the same operation: the reference's listed rows)
                assert _ok(got[name][listed], rf[listed], B[listed], c).all(), (m, s, name, "row list")
                assert np.isnan(got[name][~listed]).all(), (m, s, name, "rows outside the list")
            ls = srows[listed[srows]]; us = srows[~listed[srows]]
            assert np.array_equal(qs1[nsrank[ls]], sc[ls, None] * P1[ls]) and np.array_equal(qs1[nsrank[us]], qs0[nsrank[us]]), (m, s)
    print("step m = %d: max |gpu - ref| / (u B):" % m, " ".join("%s %.2f" % kv for kv in sorted(worst.items())))


@pytest.mark.parametrize("m", [17, 4099])
def test_step_stop_word_stamp(hip, m):
    """The step of iteration `it` runs with the stop word 0 or it + 2 (set by this iteration's k_xtb_small: its update stands) and writes nothing with
    it + 1 or a smaller non-zero stamp."""
    host, L = hip
    rng = np.random.default_rng(6000 + m)
    it = 6
    y0 = rng.standard_normal(m); sc = rng.uniform(0.5, 2.0, m)
    R, P, T, Y = [rng.standard_normal((m, 16)) for _ in range(4)]
    nsrank, ns = _sranks(m, "half", rng)
    qs0 = rng.standard_normal((ns, 16))
    mats = _step_mats(16, rng)
    ran = _step(L, it, mats, 0, y0, R, P, T, sc, nsrank, ns, Y=Y, qs=qs0)
    before = (y0, R, P, Y, qs0)
    assert all(a.tobytes() != b.tobytes() for a, b in zip(ran, before))
    for done, runs in ((it + 2, True), (0, True), (it + 1, False), (it, False), (1, False)):
        out = _step(L, it, mats, done, y0, R, P, T, sc, nsrank, ns, Y=Y, qs=qs0)
        for a, b, c in zip(out, ran, before):
            assert a.tobytes() == (b if runs else c).tobytes(), (m, done)
    # the set-up pass (it = -1): stamp 1 = it + 2 runs
    out = _step(L, -1, mats, 1, y0, R, P, T, sc, nsrank, ns, Y=Y, qs=qs0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(out, ran))


def test_step_refuses_bad_arguments(hip):
    host, L = hip
    m = 20
    z = np.zeros((m, 16)); y = np.zeros(m); sc = np.ones(m); mats = np.zeros((4, 16, 16)); qs = np.zeros((m, 16))
    nsr = np.full(m, -1, dtype=np.int32)
    both = nsr.copy(); both[3] = both[4] = 0
    call = lambda mm, it, ns_arr, ns, lst, nl: L.dkmc_xtb_test_step(mm, it, _p(mats), 0, _p(y), _p(z.copy()), _p(z.copy()), _p(z), _p(sc), _p(ns_arr), ns,
                                                                     _p(lst), nl, None, _p(qs))
    for args in ((0, 0, nsr, 0, None, 0), (m, -2, nsr, 0, None, 0), (m, 0, both, 1, None, 0), (m, 0, nsr, 1, None, 0),
                 (m, 0, nsr, 0, np.array([0, 1, m], dtype=np.int32), 3), (m, 0, nsr, 0, np.array([0, 1, 1], dtype=np.int32), 3),
                 (m, 0, nsr, 0, np.array([0, 1, 2], dtype=np.int32), 0), (m, 0, nsr, 0, np.arange(m, dtype=np.int32), m + 1)):
        assert call(*args) != 0, args[:2]
        L.dkmc_clear_error()
    assert call(m, 0, nsr, 0, None, 0) == 0


# ---- the aids leave the solver alone ---------------------------------------------------------------------------------------------------------
def test_aids_leave_the_next_solve_alone(cell_2p5, hip):
    """A warm solve behind the three aids gives the bits (potentials, I_macro, sweeps) of the same sequence without them."""
    from devicekmc_amd import params as pm
    from test_gpu_precond_reference import _record, _solve_once
    host, L = hip
    p = pm.KMCParameters(); p.solve_heating_global = False
    rng = np.random.default_rng(9)

    def sequence(with_aids):
        dev, gb = _solve_once(cell_2p5, p, hip)
        first = _record(dev, gb, host)
        if with_aids:
            m = 300
            pan = [rng.standard_normal((m, 16)) for _ in range(4)]
            nsrank, ns = _sranks(m, "half", rng)
            _gram(L, pan[:3], nsrank, ns, 128)
            _small(L, 2, 16, [(ref.consistent_gram(16, 1e2, seed=1), 0.0)], 1e-300)
            _small(L, 2, 3, [(ref.branch_inputs(3, np.diag([4.0, 0.0, 9.0])), 0.0)], 1e-300)      # (a breakdown in the aid's own XCtrl)
            _step(L, 2, _step_mats(16, rng), 0, rng.standard_normal(m), pan[0], pan[1], pan[2], np.ones(m), nsrank, ns, Y=pan[3], qs=np.zeros((ns, 16)))
        dev.updatePower(gb, p, Vd)
        return first, _record(dev, gb, host)

    a0, a1 = sequence(True)
    b0, b1 = sequence(False)
    for x, y in ((a0, b0), (a1, b1)):
        assert x["m"].tobytes() == y["m"].tobytes() and x["im"] == y["im"] and x["iters"] == y["iters"]
    assert host.get_stats()["xb_fallback"] == 0
