"""The census of the live view from the fp32 image (csrc/xt_live.h: k_xtl_census_img; dkmc_debug_xtl_census_form(1)) against the census on the fp64
store (form 0) and against the host: the rule is stated on the fp64 value, the image decides a sub-block only outside a guard band of 2^-22 around the
threshold and the sub-blocks inside it are read again from the fp64 store -- so tile flags, sub-block masks and counts are EQUAL in the two forms at
every threshold, also at thresholds that sit exactly on a sub-block's largest scaled magnitude.  2.5 nm device and tile:3."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import Vd, _fresh_device, get, hip, put  # noqa: F401
from test_gpu_tile_f32 import _workload

pytestmark = pytest.mark.gpu
THETAS = (1e-4, 1e-6, 1e-10, 1e-12)


def _solved(structure, p, hip):
    """one current solve on the full view, and the host's view of the stored tunnelling block: tile list, stored masks, the solve's scaling, the largest
    scaled magnitude (sS_i |v|) sS_j of every stored sub-block -- the library's order of the two multiplications"""
    from devicekmc_amd.lib import check
    host, L = hip
    L.dkmc_set_x_tile_drop(0.0); L.dkmc_set_x_tile_drop_auto(0)
    dev, sim, gb, _ = _fresh_device(structure, p, hip)
    dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, 0); dev.updatePower(gb, p, Vd)
    st = host.get_stats()
    assert st["x_tile_stream"] == 1
    nt, nsub = C.c_longlong(0), C.c_longlong(0)
    check(L.dkmc_xt_get_tiles(C.byref(nt), C.byref(nsub), None, None))
    tiles = np.zeros((nt.value, 4), dtype=np.int32); tval = np.zeros(nsub.value * 1024)
    check(L.dkmc_xt_get_tiles(None, None, tiles.ctypes.data, tval.ctypes.data))
    ns = st["xt_ns"]
    sS = np.zeros(ns)
    check(L.dkmc_xt_get_live(1.0, None, sS.ctypes.data))
    sSp = np.zeros(256 * ((ns + 255) // 256) + 256); sSp[:ns] = sS
    B = np.abs(tval.reshape(-1, 32, 32))
    tiles = tiles.astype(np.int64)
    submax = np.zeros(nsub.value); sub_tile = np.zeros(nsub.value, dtype=np.int64); sub_bit = np.zeros(nsub.value, dtype=np.int64)
    for t, (k, w, mask, soff) in enumerate(tiles):
        sl = 0
        for q in range(8):
            if (int(mask) >> q) & 1:
                submax[soff + sl] = ((sSp[32 * k:32 * k + 32, None] * B[soff + sl]) * sSp[None, 256 * w + 32 * q:256 * w + 32 * q + 32]).max()
                sub_tile[soff + sl] = t; sub_bit[soff + sl] = q
                sl += 1
    return dict(dev=dev, gb=gb, p=p, tiles=tiles, submax=submax, sub_tile=sub_tile, sub_bit=sub_bit, nsub_t=np.array([bin(int(m)).count("1") for m in tiles[:, 2]]))


@pytest.fixture(scope="module", params=["2.5nm", "tile:3"])
def solved(request, cell_2p5, dev_7p5, hip):
    """Computed once per device, shared, left unchanged (every case below only reads the resident X)."""
    host, L = hip
    structure, p = _workload(request.param, cell_2p5, dev_7p5)
    p.solve_heating_global = False
    try:
        s = _solved(structure, p, hip)
    finally:
        L.dkmc_set_x_tile_drop_auto(1)
    s["name"] = request.param
    return s


def _census(L, s, theta, form):
    """(tile flags, sub-block masks, the three counts as the solve reports them, sub-blocks read again) of one form"""
    from devicekmc_amd.lib import check
    nt = len(s["tiles"])
    flags = np.zeros(nt, dtype=np.int32); masks = np.zeros(nt, dtype=np.int32)
    L.dkmc_debug_xtl_census_form(form)
    check(L.dkmc_xt_get_live(theta, flags.ctypes.data, None))
    re0 = L.dkmc_debug_xtl_census_reread()
    check(L.dkmc_xt_get_live_masks(theta, masks.ctypes.data))
    re1 = L.dkmc_debug_xtl_census_reread()
    assert re0 == re1
    live = flags != 0
    own = sum(bin(int(m) & 0xff).count("1") for m in masks)
    return flags, masks, (int(live.sum()), int(s["nsub_t"][live].sum()), own), re1


def _host(s, theta):
    """host masks of the sub-blocks live on their own, per tile, and which sub-blocks sit within 1e-12 relative of theta (theirs are not compared)"""
    nt = len(s["tiles"])
    own = s["submax"] >= theta
    near = np.abs(s["submax"] - theta) <= 1e-12 * theta
    masks = np.zeros(nt, dtype=np.int64)
    np.bitwise_or.at(masks, s["sub_tile"][own], 1 << s["sub_bit"][own])
    near_t = np.zeros(nt, dtype=bool); near_t[s["sub_tile"][near]] = True
    return masks, near_t


def _check(L, s, theta, want_reread):
    """want_reread: True / False -- the image form read sub-blocks again / none; None -- no statement"""
    f0, m0, c0, r0 = _census(L, s, theta, 0)
    f1, m1, c1, r1 = _census(L, s, theta, 1)
    print("%s theta %.17g: tiles live %d of %d, sub-blocks in them %d, live on their own %d; read again from the fp64 store %d" % ((s["name"], theta, c1[0], len(f1)) + c1[1:] + (r1,)))
    assert np.array_equal(f0, f1) and np.array_equal(m0, m1) and c0 == c1, (theta, c0, c1)
    assert r0 == 0
    if want_reread is not None:
        assert (r1 > 0) if want_reread else (r1 == 0), (theta, r1)
    hm, near_t = _host(s, theta)
    assert near_t.sum() <= 3
    assert np.array_equal(m1[~near_t].astype(np.int64) & 0xff, hm[~near_t]), theta
    assert np.array_equal(f1[~near_t] != 0, hm[~near_t] != 0), theta


def test_image_census_equals_the_fp64_census_and_the_host(solved, hip):
    host, L = hip
    was = L.dkmc_debug_xtl_census_form(0)
    try:
        for theta in THETAS:
            _check(L, solved, theta, False if theta == 1e-4 else None)          # (1e-4: nothing sits in the band there)
    finally:
        L.dkmc_debug_xtl_census_form(was)


def test_thresholds_on_a_sub_blocks_largest_magnitude(solved, hip):
    """theta = the exact scaled maximum of three sub-blocks (the quartiles of the non-zero maxima) and its two neighbours in fp64: the smallest case in
    which the band can go wrong.  The forms agree, and the image form has read those sub-blocks again from the fp64 store."""
    host, L = hip
    s = solved
    nz = np.flatnonzero(s["submax"] > 0)
    order = nz[np.argsort(s["submax"][nz])]
    chosen = [order[len(order) // 4], order[len(order) // 2], order[(3 * len(order)) // 4]]
    was = L.dkmc_debug_xtl_census_form(0)
    try:
        for sb in chosen:
            v = float(s["submax"][sb])
            for theta in (v, float(np.nextafter(v, np.inf)), float(np.nextafter(v, 0.0))):
                _check(L, s, theta, True)
    finally:
        L.dkmc_debug_xtl_census_form(was)


def test_a_solve_is_the_same_with_either_form(solved, hip):
    """One solve on the live view at 1e-10 per form, both from a zero start on the same state: the same report (counts, bytes, sweeps) and the same
    potentials, bit for bit."""
    from devicekmc_amd.lib import check
    host, L = hip
    s = solved
    out = []
    was = L.dkmc_debug_xtl_census_form(0)
    try:
        L.dkmc_set_x_tile_drop(1e-10); L.dkmc_set_current_warm_start(0)
        for form in (0, 1):
            L.dkmc_debug_xtl_census_form(form)
            put(s["gb"], "atom_virtual_potentials", np.zeros(s["dev"].N_atom + 2))
            s["dev"].updatePower(s["gb"], s["p"], Vd)
            info = (C.c_longlong * 8)(); ms = (C.c_double * 2)()
            check(L.dkmc_get_x_tile_live_info(info, ms))
            st = host.get_stats()
            out.append((list(info), st["cg_iters_X"], st["cg_rr_X"], get(s["gb"], "atom_virtual_potentials").copy()))
    finally:
        L.dkmc_set_x_tile_drop(0.0); L.dkmc_set_current_warm_start(1); L.dkmc_debug_xtl_census_form(was)
    (i0, it0, rr0, m0), (i1, it1, rr1, m1) = out
    assert i0 == i1 and i0[1] > 0 and it0 == it1 > 0 and rr0 == rr1 and np.array_equal(m0, m1), (i0, i1, it0, it1)
