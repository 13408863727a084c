"""The test aids of the block-CG's Gram, s x s and panel-step kernels (dkmc_xtb_test_gram / _small / _step): declared in the debug header, defined in
csrc/xtb.hip, bound in lib.py; and the host reference the GPU tests use (tests/block_cg_algebra_ref.py), validated on a numpy fp64 restatement of
k_xtb_small: the identities (i) - (v) hold within their derived counts, every negative control is rejected, and the crafted inputs of the decision and
breakdown branches give the stated outcomes.  No GPU: nothing is loaded."""
import ctypes
import os
import re

import numpy as np
import pytest

import block_cg_algebra_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dkmc_xtb_test_gram", "dkmc_xtb_test_small", "dkmc_xtb_test_step")
S_ALL = (1, 2, 3, 8, 15, 16)
KAPPAS = (1e2, 1e4, 1e6)


def _text(*p):
    return open(os.path.join(ROOT, *p)).read()


def test_aids_are_declared_defined_and_bound():
    from devicekmc_amd import lib
    raw = _text("include", "devicekmc_hip_debug.h")
    dbg = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    pub = re.sub(r"/\*.*?\*/", " ", _text("include", "devicekmc_hip.h"), flags=re.S)
    src = _text("devicekmc_amd", "csrc", "xtb.hip")
    nargs = {"dkmc_xtb_test_gram": 10, "dkmc_xtb_test_small": 8, "dkmc_xtb_test_step": 15}
    for n in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % n, dbg)
        assert m and len(m.group(1).split(",")) == nargs[n], n
        assert n not in pub, n                                           # a test aid, not part of the drop-in surface
        d = re.search(r'extern\s+"C"\s+int\s+%s\s*\(([^)]*)\)' % n, src)
        assert d and len(d.group(1).split(",")) == nargs[n], n
        res, args = lib.SYMBOLS[n]
        assert res is ctypes.c_int and len(args) == nargs[n], n
    assert lib.SYMBOLS["dkmc_xtb_test_small"][1][5] == ctypes.POINTER(lib.dkmc_xtb_ctrl)
    # the header documents the word map of the Gram matrices and the order of the six
    assert "gfin[g * 256 + 64 * (i / 4) + 16 * (i % 4) + j]" in raw and "P'T, P'R, T'R, T'T, R'R, P'P" in raw
    # the aids stand beside dkmc_xtb_check_product and have scratch slots of their own
    assert src.index("dkmc_xtb_check_product(int width") < src.index("dkmc_xtb_test_gram(int m")
    assert "S_XTB_ALG_PANELS" in _text("devicekmc_amd", "csrc", "common.h")


def test_ctrl_mirror_matches_the_kernels_struct():
    from devicekmc_amd import lib
    def fields(text, head, tail):
        body = text[text.index(head) + len(head):]
        body = body[:body.index(tail)]
        out = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                typ, rest = decl.split(None, 1)
                out += [(typ, f.strip()) for f in rest.split(",")]
        return out
    kern = fields(_text("devicekmc_amd", "csrc", "xtiles.h"), "struct XCtrl {", "}")
    head = fields(_text("include", "devicekmc_hip_debug.h"), "typedef struct dkmc_xtb_ctrl {", "}")
    assert kern == head and len(kern) == 10
    got = []
    for name, typ in lib.dkmc_xtb_ctrl._fields_:
        base, n = (typ._type_, typ._length_) if hasattr(typ, "_length_") else (typ, 0)
        got.append(({ctypes.c_double: "double", ctypes.c_int: "int"}[base], name + ("[%d]" % n if n else "")))
    assert got == kern
    assert ctypes.sizeof(lib.dkmc_xtb_ctrl) == 2 * 8 + 10 * 4


def test_word_map_round_trips_and_is_the_accumulator_map():
    G = np.arange(256, dtype=np.float64).reshape(16, 16)
    w = ref.to_kernel(G)
    assert np.array_equal(ref.from_kernel(w), G) and sorted(ref.KMAP) == list(range(256))
    for u in range(4):                                                  # register u of lane l holds entry (l / 16 + 4 u, l % 16)
        for l in range(64):
            assert w[64 * u + l] == G[l // 16 + 4 * u, l % 16]
    b = ref.gram_block([G + 1000 * g for g in range(6)], abort=1.0)
    assert len(b) == ref.GSTR and b[-1] == 1.0 and b[256 * 4 + 64 * 1 + 16 * 2 + 3] == 4000 + 16 * 6 + 3


def _emulated(s, kappa, it=3):
    G6 = ref.consistent_gram(s, kappa, seed=400000 + 1000 * s + int(round(np.log10(kappa))))
    mats, ctrl = ref.small_fp64(it, s, [(G6, 0.0)], 1e-300, ref.new_ctrl(), np.full((4, 16, 16), 7.0))
    return G6, mats, ctrl


@pytest.mark.parametrize("s", S_ALL)
def test_identities_hold_for_an_fp64_restatement_and_reject_the_controls(s):
    for kappa in KAPPAS:
        G6, mats, ctrl = _emulated(s, kappa)
        for G in G6:                                                     # the contract of xtb_mm: zero outside s x s
            assert not G[s:, :].any() and not G[:, s:].any()
        ex = ref.exact_algebra(s, G6)
        assert ex["cond_T"] <= 1e6 and ex["cond_G"] <= 1e6, (s, kappa, ex["cond_T"], ex["cond_G"])
        ids = ref.identities(s, G6, mats, ctrl["rr"][0])
        for name, (r, B, c) in ids.items():
            assert ref.ok(r, B, c), (s, kappa, name, ref.ratio(r, B), c)   # (ok() also asserts c u <= 1e-12: the input condition of (v))
        assert ref.shape_ok(s, mats)
        assert ctrl["iters"] == 4 and ctrl["rr"][0] == ctrl["rr"][1] and ctrl["done"] == 0 and ctrl["done_local"] == 0 and ctrl["pad"] == [0, 0]
        # negative control 1: the largest entry of P'R changed by 1e-9 of itself -- (i) rejects it
        G6b = [G.copy() for G in G6]
        k = np.unravel_index(np.argmax(np.abs(G6b[1])), (16, 16)); G6b[1][k] *= 1 + 1e-9
        r, B, c = ref.identities(s, G6b, mats, ctrl["rr"][0])["i"]
        assert not ref.ok(r, B, c), (s, kappa)
        # negative control 2: M3 with the wrong sign -- (iii) rejects it
        bad = mats.copy(); bad[3] = -bad[3]
        r, B, c = ref.identities(s, G6, bad, ctrl["rr"][0])["iii"]
        assert not ref.ok(r, B, c), (s, kappa)
        # ... and a transposed W (s > 1) is no upper triangle
        if s > 1:
            bad = mats.copy(); bad[1] = bad[1].T.copy()
            assert not ref.shape_ok(s, bad)


def test_branch_inputs_give_the_stated_outcomes():
    s, pre = 3, np.full((4, 16, 16), 7.0)
    run = lambda it, G6, tol2, **kw: ref.small_fp64(it, s, [(G6, 0.0)], tol2, ref.new_ctrl(**kw), pre)
    # stop test: rr against tol2 for it >= 0, sqrt(rr) for it = -1, a factor 4 either side
    for it, tol2, above, below in ((2, 100.0, 400.0, 25.0), (-1, 0.01, 0.04 ** 2, 0.0025 ** 2)):
        for rr, stops in ((above, False), (below, True)):
            G6 = ref.branch_inputs(s, np.diag([rr, 5.0, 7.0]))
            mats, c = run(it, G6, tol2)
            assert c["done"] == (it + 2 if stops else 0) and c["done_local"] == 0 and c["rr"] == [rr, rr] and c["iters"] == it + 1
            assert not mats[0].any() and not mats[2].any() and not mats[3].any()
            assert np.allclose(np.diag(-mats[1])[:s], 1 / np.sqrt([rr, 5.0, 7.0]), rtol=2 * ref.U, atol=0)
            mats, c = run(it, G6, tol2, sharded=1)
            assert c["done"] == 0 and c["done_local"] == (1 if stops else 0)
    # indefinite with a positive diagonal: the directions are only rescaled, the loop goes on
    RR = ref.indefinite_rr(s)
    assert np.all(np.diag(RR) > 0) and np.linalg.eigvalsh(RR).min() < 0
    mats, c = run(4, ref.branch_inputs(s, RR), 1e-300, pad=[0, 5])
    assert c["pad"] == [0, 6] and c["done"] == 0
    assert np.array_equal(-mats[1][:s, :s], np.diag(1 / np.sqrt(np.diag(RR))))
    # a zero / negative diagonal entry ends the loop behind this iteration's update
    for d in (0.0, -1.0):
        mats, c = run(4, ref.branch_inputs(s, np.diag([4.0, d, 9.0])), 1e-300)
        assert c["pad"][0] == 2 and c["done"] == 6 and not mats[1].any() and not mats[2].any() and not mats[3].any()
    # P'T with a non-positive pivot (first, later): stop BEFORE the update, nothing written
    for PT in (np.diag([-1.0, 1.0, 1.0]), np.diag([0.0, 1.0, 1.0]), np.array([[1.0, 2, 0], [2, 1, 0], [0, 0, 1]])):
        mats, c = run(4, ref.branch_inputs(s, np.diag([4.0, 5.0, 9.0]), PT=PT), 1e-300)
        assert c["pad"][0] == 1 and c["done"] == 5 and np.array_equal(mats, pre) and c["iters"] == 0
    # an abort word of any rank (nrg > 1); a preset stop word
    G6 = ref.branch_inputs(s, np.diag([4.0, 5.0, 9.0]))
    for it in (-1, 3):
        mats, c = ref.small_fp64(it, s, [(G6, 0.0), (G6, 1.0)], 1e-300, ref.new_ctrl(), pre)
        assert c["aborted"] == 1 and c["done"] == max(it + 1, 1) and np.array_equal(mats, pre)
    mats, c = run(3, G6, 1e-300, done=2)
    assert np.array_equal(mats, pre) and c == ref.new_ctrl(done=2)


def test_w_identity_accepts_the_factor_and_rejects_a_scaled_one():
    rng = np.random.default_rng(5)
    s = 8
    X = rng.standard_normal((40, s)); G = X.T @ X
    W = np.linalg.inv(np.linalg.cholesky(G)).T
    r, B, c = ref.w_identity(s, G, W)
    assert ref.ok(r, B, c)
    r, B, c = ref.w_identity(s, G, W * (1 + 1e-9))
    assert not ref.ok(r, B, c)
