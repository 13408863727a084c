"""The gap analysis on the device (dkmc_find_gaps, csrc/gaps.hip) against the host reference gap_ref.py: island graph, chain, direct gap and info --
every integer and every d2 -- with np.array_equal; the number of Boruvka rounds against the reference's synchronous model."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_ref as cr
import gap_ref as gr
from analysis_support import _dev, hip  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = (50.0, 20.0, 20.0)


@pytest.fixture(autouse=True)
def _default_skip(hip):
    yield
    hip[1].dkmc_debug_set_gap_cell_skip(1)


def run_raw(hip, label, x, y, z, lattice, pbc, n_left, n_right, r_max):
    """the raw entry point on host arrays -> (edges, chain, info)"""
    host, _ = hip
    return host.find_gaps(_dev(label, np.int32), _dev(x, np.float64), _dev(y, np.float64), _dev(z, np.float64), lattice, pbc, n_left, n_right, r_max)


def check_raw(hip, label, x, y, z, lattice, pbc, n_left, n_right, r_max):
    ref = gr.analyse(label, x, y, z, lattice, pbc, n_left, n_right, r_max)
    got = run_raw(hip, label, x, y, z, lattice, pbc, n_left, n_right, r_max)
    gr.assert_equal(*got, ref)
    return got, ref


def _bytes(res):
    edges, chain, info = res
    return b"".join(edges[k].tobytes() for k in gr.EDGES) + b"".join(chain[k].tobytes() for k in gr.CHAIN) + repr([info[k] for k in gr.INFO_PINNED]).encode()


# ---- the golden device ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev_2p5(hip, cell_2p5):
    from devicekmc_amd import params as pm
    host, _ = hip
    p = pm.KMCParameters()
    dev = host.Device(cell_2p5, p)
    return dev, dev.make_gpubuf("cuda:0"), p, dev.site_element.copy()


@pytest.fixture(scope="module")
def planted(hip, dev_2p5):
    """labels of Device.find_clusters for a planted filament, as a device tensor and a host array; one labelling per planting"""
    import torch
    dev, gb, p, el0 = dev_2p5
    done = {}

    def get(r, skip):
        if (r, skip) not in done:
            el2, _ = cr.plant_filament(el0, dev.site_x, dev.site_y, dev.site_z, r, skip)
            try:
                dev.site_element = el2
                gb.t["site_element"].copy_(torch.as_tensor(el2))
                label, _, info = dev.find_clusters(gb)
                done[(r, skip)] = (dev._cluster_label.clone(), label.copy(), info)
            finally:
                dev.site_element = el0.copy()
                gb.t["site_element"].copy_(torch.as_tensor(el0))
        return done[(r, skip)]
    return get


def _contacts(dev, p):
    return dev.get_num_in_contacts(p.num_atoms_first_layer, "left"), dev.get_num_in_contacts(p.num_atoms_first_layer, "right")


def _worst_hop(chain):
    k = int(np.argmax(chain["d2"]))
    return int(chain["from_site"][k]), int(chain["to_site"][k])


@pytest.mark.parametrize("pbc", [0, 1])
@pytest.mark.parametrize("r_max", [6.0, 10.0, 16.0])
@pytest.mark.parametrize("r,skip", [(3.0, (25, 40)), (2.0, None), (3.0, (20, 30))])
def test_planted_filament_2p5(hip, dev_2p5, planted, r, skip, r_max, pbc):
    """at pbc 1 and r_max 16 the periodic axes (25.575 A) have a single cell, at 10 two"""
    host, _ = hip
    dev, gb, p, _ = dev_2p5
    tlabel, label, _ = planted(r, skip)
    nl, nr = _contacts(dev, p)
    ref = gr.analyse(label, dev.site_x, dev.site_y, dev.site_z, p.lattice, pbc, nl, nr, r_max)
    edges, chain, info = host.find_gaps(tlabel, gb.site_x, gb.site_y, gb.site_z, p.lattice, pbc, nl, nr, r_max)
    print(r, skip, r_max, pbc, info)
    gr.assert_equal(edges, chain, info, ref)
    if pbc == 0 and (r, skip) == (3.0, (25, 40)):
        assert info["n_components"] == 70
        if r_max == 6.0:
            assert (info["status"], info["n_edges"], info["direct"]) == (0, 55, None) and info["bottleneck_d2"] == np.inf
        else:
            assert (info["n_edges"], info["status"], info["n_hops"]) == (69, 1, 8) and _worst_hop(chain) == (3003, 3343)
            assert info["direct"] is None if r_max == 10.0 else info["direct"][:2] == (2850, 3704)
    if pbc == 0 and (r, skip) == (2.0, None):
        assert info["n_hops"] == 1 and (int(chain["from_site"][0]), int(chain["to_site"][0])) == (1776, 2010) == info["direct"][:2]
        assert info["bottleneck"] == info["direct"][2]


@pytest.mark.parametrize("pbc", [0, 1])
def test_bridged_planting_2p5(hip, dev_2p5, planted, pbc):
    host, _ = hip
    dev, gb, p, _ = dev_2p5
    tlabel, label, cinfo = planted(3.0, None)
    assert cinfo["bridged"] == 1
    nl, nr = _contacts(dev, p)
    ref = gr.analyse(label, dev.site_x, dev.site_y, dev.site_z, p.lattice, pbc, nl, nr, 10.0)
    edges, chain, info = host.find_gaps(tlabel, gb.site_x, gb.site_y, gb.site_z, p.lattice, pbc, nl, nr, 10.0)
    gr.assert_equal(edges, chain, info, ref)
    assert info["status"] == 2 and info["bottleneck_d2"] == 0.0 and info["n_hops"] == 0 and len(chain["d2"]) == 0 and info["direct"] is None
    assert info["n_components"] == 65 and info["n_edges"] == 64 == len(edges["d2"])                  # the forest is still returned


def test_device_find_gaps(hip, dev_2p5, cell_2p5):
    """Device.find_gaps returns and stores the same objects; with no find_clusters before it, it runs one"""
    host, _ = hip
    _, gb, p, _ = dev_2p5
    dev = host.Device(cell_2p5, p)
    assert not hasattr(dev, "site_cluster")
    edges, chain, info = dev.find_gaps(gb, r_max=10.0)
    assert dev.gap_edges is edges and dev.gap_chain is chain and dev.gap_info is info
    assert dev.cluster_info["n_components"] == 79 == info["n_components"]
    nl, nr = _contacts(dev, p)
    ref = gr.analyse(dev.site_cluster, dev.site_x, dev.site_y, dev.site_z, p.lattice, p.pbc, nl, nr, 10.0)
    gr.assert_equal(edges, chain, info, ref)
    # the labels of an earlier find_clusters are the ones used
    dev.find_clusters(gb, members=host.VACANCY)
    e2, c2, i2 = dev.find_gaps(gb, r_max=6.0)
    gr.assert_equal(e2, c2, i2, gr.analyse(dev.site_cluster, dev.site_x, dev.site_y, dev.site_z, p.lattice, p.pbc, nl, nr, 6.0))
    assert i2["n_components"] == 83 and dev.gap_info is i2


# ---- a synthetic integer lattice ----------------------------------------------------------------------------------------------------------
def _integer_lattice():
    """Sites on integer coordinates.  Two contact slabs (2 x 6 x 6) 32 apart, a row of eight 2 x 2 x 2 islands between them with the gaps
    3 | 2 3 2 4 2 3 2 | 3 -- pairs, then quadruples, then all of them merge: three contracting rounds -- and two islands A, B beside the third one
    of the row at distance 3, numbered before the row.  Facing 2 x 2 faces give four tied candidates per gap.  The other lattice points are
    non-members.  Order of the sites: left slab, A, B, the row, non-members, right slab."""
    cube = lambda x0, y0, z0: [(x0 + i, y0 + j, z0 + k) for i in (0, 1) for j in (0, 1) for k in (0, 1)]
    slab = lambda x0: [(x0 + i, j, k) for i in (0, 1) for j in range(6) for k in range(6)]
    starts, face = [], 1                                                            # face: the last occupied plane so far
    for gap in (3, 2, 3, 2, 4, 2, 3, 2):
        starts.append(face + gap)
        face += gap + 1
    row = [cube(s, 2, 2) for s in starts]
    x_right = face + 3
    third = starts[2]
    groups = [slab(0), cube(third, -2, 2), cube(third, 6, 2)] + row
    used = {q for g in groups for q in g} | set(slab(x_right))
    filler = [(i, j, k) for i in range(x_right + 2) for j in range(-2, 8) for k in range(6) if (i, j, k) not in used]
    pts = [q for g in groups for q in g] + filler + slab(x_right)
    xyz = np.array(pts, dtype=np.float64)
    N = len(pts)
    label = np.full(N, -1, dtype=np.int32)
    at = 0
    for g in groups:
        label[at:at + len(g)] = at
        at += len(g)
    label[N - 72:] = N - 72
    label[at:at + 5] = [N, N + 7, 2 ** 31 - 1, -2, -2 ** 31]                       # not members: labels outside 0 ... N - 1
    return label, xyz[:, 0].copy(), xyz[:, 1].copy(), xyz[:, 2].copy(), 72, 72


def test_integer_lattice(hip):
    label, x, y, z, nl, nr = _integer_lattice()
    N = len(label)
    assert 1500 < N < 3000
    lat = (100.0, 100.0, 100.0)
    # what the case is built for, read off the reference's candidates
    (a, b, d2, na, nb), _ = gr.candidates(label, x, y, z, lat, 0, nl, nr, 32.0)
    assert len(d2) - len(np.unique(d2)) > 100                                      # exact ties
    first = {}
    for k in range(len(d2)):                                                        # key order: every node's first edge is its pick
        first.setdefault(int(na[k]), k); first.setdefault(int(nb[k]), k)
    picks = {n: int(nb[k]) if int(na[k]) == n else int(na[k]) for n, k in first.items()}
    lost = [c for c in picks if sum(1 for n in picks if picks[n] == c and n < c and picks[c] != n) >= 2]
    assert lost, picks                                                              # a node that picks another while two smaller ones pick it
    for k in first.values():                                                        # a pick is the smallest (a, b) among its node's ties
        tied = np.flatnonzero(d2 == d2[k])
        assert len(tied) >= 4
    (edges, chain, info), ref = check_raw(hip, label, x, y, z, lat, 0, nl, nr, 32.0)
    assert info["rounds"] == ref[2]["rounds"] >= 4                                 # three contracting rounds + the one without a candidate
    assert info["n_components"] == 12 and info["n_edges"] == 11 and info["status"] == 1 and info["n_hops"] == 9
    assert info["direct"][2] == 32.0 and info["bottleneck"] == 4.0                 # the slabs are r_max apart exactly: included
    assert np.array_equal(chain["d2"], [9.0, 4.0, 9.0, 4.0, 16.0, 4.0, 9.0, 4.0, 9.0])
    # a cell grid of many cells, no direct gap within reach; and one that stops short of the widest gap
    (_, chain, info), _ = check_raw(hip, label, x, y, z, lat, 0, nl, nr, 4.5)
    assert info["status"] == 1 and info["direct"] is None and info["n_hops"] == 9
    (_, _, info), _ = check_raw(hip, label, x, y, z, lat, 0, nl, nr, 3.5)
    assert info["status"] == 0 and info["n_edges"] == 10 and info["bottleneck_d2"] == np.inf
    # periodic in y, z with a lattice that brings A and B (y = -2 ... 7) next to each other through the boundary
    check_raw(hip, label, x, y, z, (100.0, 11.0, 50.0), 1, nl, nr, 4.5)


# ---- random point sets: every shape of the cell grid ------------------------------------------------------------------------------------
def _random_points(seed, n=1500, n_labels=40, frac=0.5, ends=0):
    """ends > 0: the labels 5 ... 9 occur among the last `ends` sites only and not among the first: with ends sites per contact set nothing is bridged,
    node L is scattered over the whole box and node R is small"""
    rng = np.random.default_rng(seed)
    x, y, z = rng.random(n) * BOX[0], rng.random(n) * BOX[1], rng.random(n) * BOX[2]
    lab = rng.integers(0, n_labels, n)
    if ends:
        lab[:n - ends] = np.where((lab[:n - ends] >= 5) & (lab[:n - ends] <= 9), lab[:n - ends] + 10, lab[:n - ends])
        lab[n - ends:] = 5 + lab[n - ends:] % 5
    label = np.where(rng.random(n) < frac, lab * 7 % n, -1).astype(np.int32)       # any value in 0 ... N - 1 names a component
    return label, x, y, z


@pytest.mark.parametrize("pbc", [0, 1])
@pytest.mark.parametrize("r_max", [1.5, 3.0, 8.0, 12.0, 25.0, 80.0])
def test_random_points(hip, r_max, pbc):
    """periodic axes of 13, 6, 2 and 1 cells, r_max above the periodic box and above the whole box; members of one node scattered over the cells"""
    label, x, y, z = _random_points(int(r_max * 10) + pbc, ends=30)
    (_, _, info), _ = check_raw(hip, label, x, y, z, BOX, pbc, 30, 30, r_max)
    assert info["status"] == 1 and info["direct"] is not None and info["n_edges"] >= 17


@pytest.mark.parametrize("n", [1, 2, 63, 65, 257])
def test_small_sizes(hip, n):
    label, x, y, z = _random_points(n, n=n, n_labels=5, frac=0.8)
    check_raw(hip, label, x, y, z, BOX, 1, n // 4, n // 4, 30.0)
    check_raw(hip, label, x, y, z, BOX, 0, n // 4, n // 4, 9.0)


# ---- edges of the domain ----------------------------------------------------------------------------------------------------------------------
def test_minimum_image_across_the_boundary(hip):
    x, y, z = np.array([0.0, 1.0, 0.0]), np.array([0.5, 4.0, 7.5]), np.array([0.25, 4.0, 0.25])      # 7 / 8 of the lattice apart: exact
    label = np.array([0, 1, 2], dtype=np.int32)
    (_, chain, info), _ = check_raw(hip, label, x, y, z, (10.0, 8.0, 8.0), 1, 1, 1, 3.0)
    assert info["direct"] == (0, 2, 1.0) and info["n_hops"] == 1 and info["n_edges"] == 1
    (_, chain, info), _ = check_raw(hip, label, x, y, z, (10.0, 8.0, 8.0), 0, 1, 1, 3.0)
    assert info["direct"] is None and info["status"] == 0 and info["n_edges"] == 0


def test_r_max_is_included_one_ulp_more_is_not(hip):
    lat = (10.0, 10.0, 10.0)
    for pbc in (0, 1):
        for zb, inside in ((0.0, True), (6e-8, False)):
            x, y, z = np.array([0.0, 3.0]), np.array([0.0, 4.0]), np.array([0.0, zb])
            d2 = gr.pair_d2(np.array([0]), np.array([1]), x, y, z, lat, pbc)[0]
            assert d2 == (25.0 if inside else np.nextafter(25.0, np.inf))
            (edges, _, info), _ = check_raw(hip, np.array([0, 1], dtype=np.int32), x, y, z, lat, pbc, 1, 1, 5.0)
            assert (info["n_edges"], info["status"]) == ((1, 1) if inside else (0, 0))
            assert info["direct"] == ((0, 1, 5.0) if inside else None)


def test_degenerate_inputs(hip):
    import torch
    host, L = hip
    label, x, y, z = _random_points(3, n=400, n_labels=12)
    # no member at all
    (edges, chain, info), _ = check_raw(hip, np.full(400, -1, dtype=np.int32), x, y, z, BOX, 1, 50, 50, 10.0)
    assert info["n_components"] == 0 and info["status"] == 0 and len(edges["d2"]) == 0 and len(chain["d2"]) == 0 and info["bottleneck_d2"] == np.inf
    # labels >= N (and below 0) are not members, and nothing is read through them
    wild = label.copy()
    wild[::3] = 400
    wild[1::9] = 2 ** 31 - 1
    (_, _, info), ref = check_raw(hip, wild, x, y, z, BOX, 0, 50, 50, 10.0)
    assert info["n_components"] == ref[2]["n_components"] <= 12
    # one contact set empty: no chain, no direct gap, the forest all the same
    (edges, chain, info), _ = check_raw(hip, label, x, y, z, BOX, 1, 50, 0, 10.0)
    assert info["status"] == 0 and info["direct"] is None and len(chain["d2"]) == 0 and info["n_edges"] > 0
    (edges, chain, info), _ = check_raw(hip, label, x, y, z, BOX, 1, 0, 0, 10.0)
    assert info["status"] == 0 and info["n_edges"] == 11
    # contact counts beyond N are clamped: everything is one node
    (_, _, info), _ = check_raw(hip, label, x, y, z, BOX, 1, 10 ** 6, -5, 10.0)
    assert info["n_edges"] == 0 and info["status"] == 0
    # N == 0
    e = torch.empty(0, dtype=torch.float64, device="cuda:0")
    edges, chain, info = host.find_gaps(torch.empty(0, dtype=torch.int32, device="cuda:0"), e, e, e, BOX, 1, 0, 0, 10.0)
    assert info["n_components"] == 0 and info["status"] == 0 and info["n_edges"] == 0 and len(edges["d2"]) == 0 and len(chain["d2"]) == 0


def test_capacity(hip):
    _, L = hip
    label, x, y, z, nl, nr = _integer_lattice()
    (edges, chain, info), _ = check_raw(hip, label, x, y, z, (100.0, 100.0, 100.0), 0, nl, nr, 4.5)
    assert info["n_edges"] == 11 and info["n_hops"] == 9
    a, d2, rows = np.full(8, -9, dtype=np.int32), np.full(8, -9.0), C.c_int(-1)
    assert L.dkmc_copy_gap_edges(5, a.ctypes.data_as(C.c_void_p), None, None, None, d2.ctypes.data_as(C.c_void_p), C.byref(rows)) == 0
    assert rows.value == 5 and np.array_equal(a[:5], edges["site_a"][:5]) and np.array_equal(d2[:5], edges["d2"][:5]) and (a[5:] == -9).all()
    assert L.dkmc_copy_gap_edges(0, None, None, None, None, None, C.byref(rows)) == 0 and rows.value == 0
    t = np.full(4, -9, dtype=np.int32)
    assert L.dkmc_copy_gap_chain(1, None, t.ctypes.data_as(C.c_void_p), None, C.byref(rows)) == 0
    assert rows.value == 1 and t[0] == chain["to_site"][0] and (t[1:] == -9).all()
    assert L.dkmc_copy_gap_chain(10 ** 6, None, None, None, None) == 0
    i8 = (C.c_longlong * 8)()
    assert L.dkmc_get_gap_info(i8, None) == 0 and (i8[1], i8[3]) == (info["n_edges"], info["n_hops"])


def test_bad_arguments(hip):
    host, L = hip
    label, x, y, z = _random_points(6, n=100)
    t = [_dev(label, np.int32)] + [_dev(v, np.float64) for v in (x, y, z)]
    lat = np.array(BOX)
    lp = lat.ctypes.data_as(C.c_void_p)
    p = [host._ptr(v) for v in t]
    assert L.dkmc_find_gaps(100, p[1], p[2], p[3], lp, 1, p[0], 10, 10, 5.0) == 0
    for r_max in (0.0, -1.0, float("nan"), float("inf")):
        assert L.dkmc_find_gaps(100, p[1], p[2], p[3], lp, 1, p[0], 10, 10, r_max) == 3
        assert "dkmc_find_gaps" in L.dkmc_last_error().decode()
        L.dkmc_clear_error()
        assert L.dkmc_get_gap_info(None, None) != 0                                 # no results of a failed call
        L.dkmc_clear_error()
    for args in ((-1, p[1], p[2], p[3], lp, 1, p[0]), (100, None, p[2], p[3], lp, 1, p[0]), (100, p[1], p[2], p[3], lp, 1, None)):
        assert L.dkmc_find_gaps(*args, 10, 10, 5.0) == 3
        L.dkmc_clear_error()
    assert L.dkmc_find_gaps(100, p[1], p[2], p[3], lp, 1, p[0], 10, 10, 5.0) == 0 and L.dkmc_get_gap_info(None, None) == 0


def test_getters_before_any_call(hip):
    """in a fresh process: the three getters fail and name themselves"""
    code = ("import sys, ctypes as C; sys.path.insert(0, %r)\n"
            "from devicekmc_amd import lib\n"
            "L = lib.load(); r = C.c_int(0)\n"
            "calls = (('dkmc_get_gap_info', lambda: L.dkmc_get_gap_info(None, None)), ('dkmc_copy_gap_edges', lambda: L.dkmc_copy_gap_edges(4, None, None, None, None, None, C.byref(r))),\n"
            "         ('dkmc_copy_gap_chain', lambda: L.dkmc_copy_gap_chain(4, None, None, None, C.byref(r))))\n"
            "for name, call in calls:\n"
            "    rc = call()\n"
            "    assert rc == 3 and name in L.dkmc_last_error().decode(), (rc, name)\n"
            "    L.dkmc_clear_error()\n"
            "print('getters refused')\n") % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "getters refused" in out.stdout, out.stderr


# ---- repeatability and purity ---------------------------------------------------------------------------------------------------------------
def test_two_calls_same_bytes_and_the_cell_skip(hip):
    _, L = hip
    label, x, y, z = _random_points(9, n=3000, n_labels=25, frac=0.7)
    label[:400] = np.where(label[:400] >= 0, 0, -1)                                 # a slab of one node: cells the skip passes over
    label[-100:] = np.where(label[-100:] >= 0, 7, -1)                               # the right contact set is one component too: nothing is bridged
    order = np.argsort(x, kind="stable")
    x, y, z = x[order], y[order], z[order]
    ref = gr.analyse(label, x, y, z, BOX, 1, 400, 100, 6.0)
    a = run_raw(hip, label, x, y, z, BOX, 1, 400, 100, 6.0)
    b = run_raw(hip, label, x, y, z, BOX, 1, 400, 100, 6.0)
    L.dkmc_debug_set_gap_cell_skip(0)
    c = run_raw(hip, label, x, y, z, BOX, 1, 400, 100, 6.0)
    L.dkmc_debug_set_gap_cell_skip(1)
    for res in (a, b, c):
        gr.assert_equal(*res, ref)
    assert ref[2]["status"] == 1 and ref[2]["n_edges"] == 24 and ref[2]["rounds"] >= 3
    assert _bytes(a) == _bytes(b) == _bytes(c)
    assert a[2]["pairs_tested"] == b[2]["pairs_tested"] == c[2]["pairs_tested"] > 0      # only pairs of different nodes are tested: the skip saves reads


def test_call_changes_nothing_else(hip, dev_2p5):
    """site_element, site_charge, the labels and the cluster table of the find_clusters before it"""
    _, L = hip
    dev, gb, p, _ = dev_2p5
    dev.updateCharge(gb)
    _, table, cinfo = dev.find_clusters(gb)

    def state():
        cols = [np.empty(cinfo["n_components"], dtype=np.int32) for _ in range(4)] + [np.empty(cinfo["n_components"]) for _ in range(2)]
        rows = C.c_int(0)
        assert L.dkmc_copy_cluster_table(cinfo["n_components"], *[c.ctypes.data_as(C.c_void_p) for c in cols], C.byref(rows)) == 0
        return [gb.t[k].cpu().numpy().tobytes() for k in ("site_element", "site_charge", "site_x", "site_y", "site_z")] + \
               [dev._cluster_label.cpu().numpy().tobytes()] + [c.tobytes() for c in cols]

    before = state()
    for r_max in (6.0, 16.0):
        dev.find_gaps(gb, r_max=r_max)
    assert before == state() and before[6] == table["root"].tobytes()
