"""The two kernels of the one-polynomial form of the preconditioned block-CG (dkmc_set_x_poly_form; csrc/xtb.hip) on caller-given panels, through the
debug aids dkmc_xtb_test_gram1 / dkmc_xtb_test_step1 (include/devicekmc_hip_debug.h):
  k_xtb_gram1   six panels Pt, Pi, Q, U, Rt, Z of [m][16] -> Pt'Q, Pt'Rt, Q'Z, Q'U, Rt'Z, Pt'Pi, the last three symmetrised;
  k_xtb_step1   Y += Pt c (column 0), Rt += Q c, Z += U c, Pt = Z M1 + U M3 + Pt M2, Pi = Rt M1 + Q M3 + Pi M2, QS = S Pt on the tunnelling rows.
Shapes: one row, one row past a 16-row group, several workgroups with a ragged end; block widths 16 and 5 (the padding columns stay zero)."""
import ctypes as C

import numpy as np
import pytest

from devicekmc_amd.lib import check
from test_gpu_block_cg_algebra import _gram_count, _ld_gram, _natural, _ok, _p, _sranks, _step_mats, _worst
from test_gpu_parity import Vd, hip  # noqa: F401

pytestmark = pytest.mark.gpu

LD = np.longdouble
M = [1, 17, 4099]
S = [16, 5]
NG = [1, 7, 128]
NAMES = ("Pt", "Pi", "Q", "U", "Rt", "Z")
PAIRS = ((0, 2), (0, 4), (2, 5), (2, 3), (4, 5), (0, 1))                     # Pt'Q, Pt'Rt, Q'Z, Q'U, Rt'Z, Pt'Pi
SYM = (3, 4, 5)


def _ptrs(panels):
    return (C.c_void_p * 6)(*[p.ctypes.data for p in panels])


def _gram1(L, panels, ng, done=0, prefill=None):
    gfin = np.full(6 * 256, np.nan) if prefill is None else prefill.copy()
    check(L.dkmc_xtb_test_gram1(panels[0].shape[0], _ptrs(panels), ng, done, _p(gfin)))
    return gfin


def _symmetrise(G):
    G = G.copy()
    for g in SYM:
        G[g] = (G[g] + G[g].T) / 2
    return G


@pytest.mark.parametrize("s", S)
@pytest.mark.parametrize("m", M)
def test_gram_integer_panels_are_exact(hip, m, s):
    """Entries in [-8, 8]: every sum is an integer below 2^53 and (G + G') / 2 of integers is exact in fp64, so the six matrices equal the reference bit
    for bit whatever the grouping; a row counted twice, a wrong pair of panels or a transposed matrix cannot pass."""
    host, L = hip
    rng = np.random.default_rng(7000 + 16 * m + s)
    ipan = [rng.integers(-8, 9, (m, s)) for _ in range(6)]
    pan = [np.zeros((m, 16)) for _ in range(6)]
    for a, b in zip(pan, ipan):
        a[:, :s] = b
    want = np.zeros((6, 16, 16))
    for g, (x, z) in enumerate(PAIRS):
        want[g, :s, :s] = ipan[x].T @ ipan[z]
    want = _symmetrise(want)
    for ng in NG:
        got = _natural(_gram1(L, pan, ng))
        assert np.array_equal(got, want), (m, s, ng, np.argwhere(got != want)[:4])
        assert not got[:, s:, :].any() and not got[:, :, s:].any()
    twice = want.copy()
    for g, (x, z) in enumerate(PAIRS):
        twice[g, :s, :s] += np.outer(ipan[x][0], ipan[z][0])
    assert not np.array_equal(got, _symmetrise(twice))
    # a preset stop word leaves gfin as it came
    pre = np.arange(6 * 256, dtype=np.float64) + 0.5
    assert np.array_equal(_gram1(L, pan, 7, done=3, prefill=pre), pre)


@pytest.mark.parametrize("s", S)
@pytest.mark.parametrize("m", M)
def test_gram_real_panels_and_exact_symmetry(hip, m, s):
    """Standard normal entries, rows scaled by 10^uniform(-6, 6), against the long-double reference within the count of the kernel's grouping
    (test_gpu_block_cg_algebra._gram_count without S rows: a wave's chain over its rows of the chunk, the four waves, k_xtb_gred) + 1 for the addition of
    (G + G') / 2.  The three symmetrised matrices are symmetric bit for bit.  Negative control: the reference without the row of the largest scale."""
    host, L = hip
    rng = np.random.default_rng(8000 + 16 * m + s)
    scale = 10.0 ** rng.uniform(-6, 6, (m, 1))
    scale[rng.integers(0, m)] = 1e6
    pan = [np.zeros((m, 16)) for _ in range(6)]
    for a in pan:
        a[:, :s] = rng.standard_normal((m, s)) * scale
    lp = [p.astype(LD) for p in pan]
    want = np.stack([_ld_gram(lp[x], lp[z]) for x, z in PAIRS])
    B = np.stack([(np.abs(pan[x]).T @ np.abs(pan[z])).astype(LD) for x, z in PAIRS]) * LD(1 + 1e-9)
    for g in SYM:
        want[g] = (want[g] + want[g].T) / 2; B[g] = (B[g] + B[g].T) / 2
    drop = int(np.argmax(scale))
    without = want.copy()
    for g, (x, z) in enumerate(PAIRS):
        d = np.outer(lp[x][drop], lp[z][drop])
        without[g] -= (d + d.T) / 2 if g in SYM else d
    for ng in NG:
        c = _gram_count(m, 0, ng) + 1
        got = _natural(_gram1(L, pan, ng))
        good = _ok(got, want, B, c)
        print("gram1 m = %d s = %d ng = %d: |gpu - ref| = %.2f u B of %d" % (m, s, ng, _worst(got, want, B), c))
        assert good.all(), (m, s, ng, c, np.argwhere(~good)[:4], _worst(got, want, B))
        assert not _ok(got, without, B, c).all(), (m, s, ng)
        for g in SYM:
            assert got[g].tobytes() == np.ascontiguousarray(got[g].T).tobytes(), (m, s, ng, g)
        assert not got[:, s:, :].any() and not got[:, :, s:].any()


def _step1(L, it, mats, done, y0, panels, sc, nsrank, ns, qs):
    y0 = y0.copy(); panels = [p.copy() for p in panels]; qs = qs.copy()
    check(L.dkmc_xtb_test_step1(len(y0), it, _p(np.ascontiguousarray(mats)), done, _p(y0), _ptrs(panels), _p(sc), _p(nsrank), ns, _p(qs)))
    return y0, panels, qs


def _step1_reference(mats, y0, pan):
    """long double, from the ORIGINAL panels; name -> (ref, B, c) with the counts of test_gpu_block_cg_algebra._step_reference: y0 8, a chain of 16 fused
    multiply-adds on the input 17, three chains 49"""
    c, M1, M2, M3 = [x.astype(LD) for x in mats]
    a = np.abs(mats)
    l = dict(zip(NAMES, [p.astype(LD) for p in pan])); ab = dict(zip(NAMES, [np.abs(p) for p in pan]))
    up = LD(1 + 1e-9)
    return {"y0": (y0.astype(LD) + l["Pt"] @ c[:, 0], (np.abs(y0) + ab["Pt"] @ a[0][:, 0]) * up, 8),
            "Rt": (l["Rt"] + l["Q"] @ c, (ab["Rt"] + ab["Q"] @ a[0]) * up, 17),
            "Z": (l["Z"] + l["U"] @ c, (ab["Z"] + ab["U"] @ a[0]) * up, 17),
            "Pt": (l["Z"] @ M1 + l["U"] @ M3 + l["Pt"] @ M2, (ab["Z"] @ a[1] + ab["U"] @ a[3] + ab["Pt"] @ a[2]) * up, 49),
            "Pi": (l["Rt"] @ M1 + l["Q"] @ M3 + l["Pi"] @ M2, (ab["Rt"] @ a[1] + ab["Q"] @ a[3] + ab["Pi"] @ a[2]) * up, 49)}


@pytest.mark.parametrize("s", S)
@pytest.mark.parametrize("m", M)
def test_step_against_the_original_panels(hip, m, s):
    """Rt, Z, Pt, Pi and column 0 of Y against the long-double reference formed from the ORIGINAL panels and the given mats; QS bitwise sc[row] Pt_out[row]
    at the tunnelling rows; Q and U untouched; columns >= s: Rt, Z as they were, Pt, Pi zero.  Nothing is written once the stop word is set (it + 1 or an
    older stamp); it + 2 -- set by this iteration's k_xtb_small -- still runs.  Negative control: Pt formed with the updated Z."""
    host, L = hip
    rng = np.random.default_rng(9000 + 16 * m + s)
    it = 6
    y0 = rng.standard_normal(m); sc = rng.uniform(0.5, 2.0, m)
    pan = [rng.standard_normal((m, 16)) for _ in range(6)]
    nsrank, ns = _sranks(m, "half", rng) if m > 1 else (np.zeros(1, dtype=np.int32), 1)
    qs0 = rng.standard_normal((ns, 16)) + 100.0
    srows = np.flatnonzero(nsrank >= 0)
    mats = _step_mats(s, rng)
    want = _step1_reference(mats, y0, pan)
    y1, p1, qs1 = _step1(L, it, mats, 0, y0, pan, sc, nsrank, ns, qs0)
    got = dict(zip(NAMES, p1)); got["y0"] = y1
    for name, (rf, B, c) in want.items():
        good = _ok(got[name], rf, B, c)
        print("step1 m = %d s = %d %s: |gpu - ref| = %.2f u B of %d" % (m, s, name, _worst(got[name], rf, B), c))
        assert good.all(), (m, s, name, np.argwhere(~good)[:4], _worst(got[name], rf, B))
    assert got["Q"].tobytes() == pan[2].tobytes() and got["U"].tobytes() == pan[3].tobytes()
    if s < 16:
        assert got["Rt"][:, s:].tobytes() == pan[4][:, s:].tobytes() and got["Z"][:, s:].tobytes() == pan[5][:, s:].tobytes()
        assert not got["Pt"][:, s:].any() and not got["Pi"][:, s:].any()
    assert np.array_equal(qs1[nsrank[srows]], sc[srows, None] * got["Pt"][srows]), (m, s)
    rf, B, c = want["Pt"]
    assert not _ok(got["Pt"], rf + (got["Z"].astype(LD) - pan[5].astype(LD)) @ mats[1].astype(LD), B, c).all(), (m, s)
    # stop word
    ran = (y1, *p1, qs1); before = (y0, *pan, qs0)
    for done, runs in ((it + 2, True), (it + 1, False), (it, False), (1, False)):
        y2, p2, qs2 = _step1(L, it, mats, done, y0, pan, sc, nsrank, ns, qs0)
        for a, b, c_ in zip((y2, *p2, qs2), ran, before):
            assert a.tobytes() == (b if runs else c_).tobytes(), (m, s, done)


def test_aids_refuse_bad_arguments(hip):
    host, L = hip
    pan = [np.zeros((4, 16)) for _ in range(6)]
    gfin = np.zeros(6 * 256); y0 = np.zeros(4); sc = np.ones(4); nsr = np.full(4, -1, dtype=np.int32); mats = np.zeros((4, 16, 16))
    null5 = (C.c_void_p * 6)(*[p.ctypes.data for p in pan[:5]], None)
    for args in ((0, _ptrs(pan), 1, 0, _p(gfin)), (4, _ptrs(pan), 0, 0, _p(gfin)), (4, _ptrs(pan), 4097, 0, _p(gfin)), (4, null5, 1, 0, _p(gfin)), (4, _ptrs(pan), 1, 0, None)):
        assert L.dkmc_xtb_test_gram1(*args) != 0
        L.dkmc_clear_error()
    for args in ((0, 0, _p(mats), 0, _p(y0), _ptrs(pan), _p(sc), _p(nsr), 0, None), (4, -2, _p(mats), 0, _p(y0), _ptrs(pan), _p(sc), _p(nsr), 0, None),
                 (4, 0, _p(mats), 0, _p(y0), null5, _p(sc), _p(nsr), 0, None), (4, 0, _p(mats), 0, _p(y0), _ptrs(pan), _p(sc), _p(nsr), 1, _p(gfin))):
        assert L.dkmc_xtb_test_step1(*args) != 0
        L.dkmc_clear_error()
