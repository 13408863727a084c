"""The host reference of the gap analysis (gap_ref.py) by independent routes: scipy's minimum spanning tree of the node graph, the bridging verdict
of cluster_ref.analyse on brute-force indices around the bottleneck, the roles of the two sites of a pair swapped, and the numbers of the planted
filament of the 2.5 nm device.  No GPU."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import minimum_spanning_tree

import cluster_ref as cr
import gap_ref as gr

BOX = (40.0, 12.0, 12.0)


def _points(seed, n=500, n_labels=30, frac=0.6, ends=40):
    """random sites sorted by x; random labels, those of the first `ends` and of the last `ends` sites from two sets of their own (nothing bridged)"""
    rng = np.random.default_rng(seed)
    x = np.sort(rng.random(n) * BOX[0])
    y, z = rng.random(n) * BOX[1], rng.random(n) * BOX[2]
    lab = rng.integers(10, n_labels, n)
    lab[:ends] = rng.integers(0, 5, ends)
    lab[n - ends:] = rng.integers(5, 10, ends)
    label = np.where(rng.random(n) < frac, lab, -1).astype(np.int32)
    return label, x, y, z


def test_c_round():
    f = np.array([0.5, -0.5, 1.5, -1.5, 2.5, 0.49999999999999994, -0.49999999999999994, 0.0, -0.0, 3.2, -3.7, 1e300])
    assert np.array_equal(gr.c_round(f), [1.0, -1.0, 2.0, -2.0, 3.0, 0.0, -0.0, 0.0, -0.0, 3.0, -4.0, 1e300])


@pytest.mark.parametrize("pbc", [0, 1])
@pytest.mark.parametrize("r_max", [2.5, 5.0, 50.0])
def test_forest_weight_is_scipys(r_max, pbc):
    """tie-free point sets: the forest's weights are those of scipy's minimum spanning tree over the lightest candidate of every node pair"""
    label, x, y, z = _points(3 + pbc)
    (a, b, d2, na, nb), _ = gr.candidates(label, x, y, z, BOX, pbc, 40, 40, r_max)
    assert len(np.unique(d2)) == len(d2)
    edges, _, info = gr.analyse(label, x, y, z, BOX, pbc, 40, 40, r_max)
    nodes, inv = np.unique(np.concatenate([na, nb]), return_inverse=True)
    ia, ib = inv[:len(na)], inv[len(na):]
    w = {}
    for k in range(len(d2) - 1, -1, -1):                                           # descending: the lightest of a node pair is written last
        w[(min(ia[k], ib[k]), max(ia[k], ib[k]))] = d2[k]
    g = sp.coo_matrix((list(w.values()), tuple(zip(*w.keys()))), shape=(len(nodes), len(nodes))).tocsr()
    t = minimum_spanning_tree(g)
    assert np.array_equal(np.sort(t.data), edges["d2"]) and info["n_edges"] == t.nnz
    assert np.array_equal(edges["d2"], np.sort(edges["d2"])) and (edges["site_a"] < edges["site_b"]).all()
    assert np.array_equal(edges["root_a"], label[edges["site_a"]]) and np.array_equal(edges["root_b"], label[edges["site_b"]])


def _index_within(x, y, z, lattice, pbc, d2_max):
    """brute-force padded neighbour index: v in row u when d2(u, v) <= d2_max"""
    n = len(x)
    iu, iv = np.triu_indices(n, 1)
    keep = gr.pair_d2(iu, iv, x, y, z, lattice, pbc) <= d2_max
    rows = [[] for _ in range(n)]
    for u, v in zip(iu[keep], iv[keep]):
        rows[u].append(v); rows[v].append(u)
    index = np.full((n, max(1, max(len(r) for r in rows))), -1, dtype=np.int32)
    for u, r in enumerate(rows):
        index[u, :len(r)] = r
    return index


@pytest.mark.parametrize("pbc", [0, 1])
def test_bottleneck_is_where_the_cluster_analysis_turns_to_bridged(pbc):
    rng = np.random.default_rng(17 + pbc)
    n = 400
    x = np.sort(rng.random(n) * BOX[0])
    y, z = rng.random(n) * BOX[1], rng.random(n) * BOX[2]
    element = np.where(rng.random(n) < 0.5, cr.VACANCY_EL, 3).astype(np.int32)
    args = (element, None, x, [6], cr.VACANCY_BIT, 30, 30)
    label, _, cinfo = cr.analyse(_index_within(x, y, z, BOX, pbc, 1.5 ** 2), *args, with_rounds=False)
    assert cinfo["bridged"] == 0 and cinfo["n_components"] > 20
    edges, chain, info = gr.analyse(label, x, y, z, BOX, pbc, 30, 30, 50.0)
    assert info["status"] == 1 and info["n_hops"] >= 2 and info["bottleneck_d2"] == chain["d2"].max() > 1.5 ** 2
    assert info["direct"] is not None and info["direct"][2] > info["bottleneck"]
    b2 = info["bottleneck_d2"]
    assert cr.analyse(_index_within(x, y, z, BOX, pbc, b2), *args, with_rounds=False)[2]["bridged"] == 1
    assert cr.analyse(_index_within(x, y, z, BOX, pbc, np.nextafter(b2, 0.0)), *args, with_rounds=False)[2]["bridged"] == 0
    # the chain is a path: it starts in L, ends in R, and every hop leaves the island the hop before reached
    nl_nodes = {int(v) for v in label[:30] if v >= 0}
    nr_nodes = {int(v) for v in label[n - 30:] if v >= 0}
    assert int(label[chain["from_site"][0]]) in nl_nodes and int(label[chain["to_site"][-1]]) in nr_nodes
    assert np.array_equal(label[chain["to_site"][:-1]], label[chain["from_site"][1:]])
    # a chain stops being found exactly where r_max falls below the bottleneck
    assert gr.analyse(label, x, y, z, BOX, pbc, 30, 30, info["bottleneck"] * (1 - 1e-9))[2]["status"] == 0


@pytest.mark.parametrize("pbc", [0, 1])
def test_roles_of_the_two_sites(pbc, monkeypatch):
    """d2 with u and v swapped is the same bits -- exact halves of the lattice included -- and so is the whole analysis"""
    rng = np.random.default_rng(5)
    x, y, z = rng.random(300) * 40, np.round(rng.random(300) * 24) / 2, np.round(rng.random(300) * 24) / 2      # multiples of 0.5: fy = +-0.5 occurs
    iu, iv = np.triu_indices(300, 1)
    fwd, back = gr.pair_d2(iu, iv, x, y, z, BOX, pbc), gr.pair_d2(iv, iu, x, y, z, BOX, pbc)
    assert np.array_equal(fwd, back)
    if pbc:
        assert (np.abs(y[iu] - y[iv]) == 6.0).any()
    label, x, y, z = _points(8)
    ref = gr.analyse(label, x, y, z, BOX, pbc, 40, 40, 6.0)
    plain = gr.pair_d2
    monkeypatch.setattr(gr, "pair_d2", lambda a, b, *rest: plain(b, a, *rest))
    swapped = gr.analyse(label, x, y, z, BOX, pbc, 40, 40, 6.0)
    gr.assert_equal(*swapped, ref)
    assert ref[2]["n_edges"] > 10


def test_planted_filament_2p5(cell_2p5):
    """the CPU prototype's numbers: gap_x 14.396, the closest tip-to-tip pair (2850, 3704) at 14.664, eight hops, the widest (3003, 3343) at 7.660"""
    from devicekmc_amd import host, params as pm
    p = pm.KMCParameters()
    dev = host.Device(cell_2p5, p)
    nl, nr = dev.get_num_in_contacts(p.num_atoms_first_layer, "left"), dev.get_num_in_contacts(p.num_atoms_first_layer, "right")
    el, _ = cr.plant_filament(dev.site_element, dev.site_x, dev.site_y, dev.site_z, 3.0, (25, 40))
    label, _, cinfo = cr.analyse(dev.neigh_idx, el, None, dev.site_x, list(p.metals), cr.METAL | cr.VACANCY_BIT, nl, nr, with_rounds=False)
    assert round(cinfo["gap_x"], 3) == 14.396
    (_, _, d2, _, _), _ = gr.candidates(label, dev.site_x, dev.site_y, dev.site_z, p.lattice, 0, nl, nr, 10.0)
    ties = np.unique(d2, return_counts=True)[1]
    assert ties.max() >= 2                                                          # a crystal: exact ties among the candidates
    edges, chain, info = gr.analyse(label, dev.site_x, dev.site_y, dev.site_z, p.lattice, 0, nl, nr, 16.0)
    assert (info["n_components"], info["n_edges"], info["status"], info["n_hops"]) == (70, 69, 1, 8)
    k = int(np.argmax(chain["d2"]))
    assert (int(chain["from_site"][k]), int(chain["to_site"][k])) == (3003, 3343) and round(info["bottleneck"], 3) == 7.660
    assert info["direct"][:2] == (2850, 3704) and round(info["direct"][2], 3) == 14.664
    info6 = gr.analyse(label, dev.site_x, dev.site_y, dev.site_z, p.lattice, 0, nl, nr, 6.0)[2]
    assert (info6["status"], info6["n_edges"], info6["direct"]) == (0, 55, None)
