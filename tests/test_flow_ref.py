"""The host reference of the min-cut analysis (flow_ref.py) checked on its own: W, both extreme minimum cuts and the strands against the
definition (delete every subset of the interior, search) on small random graphs, hand cases, and the planted filaments of the 2.5 nm golden
device, whose figures are pinned here.  No GPU."""
import numpy as np
import pytest

import cluster_ref as cr
import cut_ref as cu
import flow_ref as fl
from analysis_support import _contacts, index_of, ladder
from analysis_support import ordered_chain as _chain
from cut_ref import planted_2p5
from flow_ref import PINNED_2P5, PINNED_2P5_ROUNDS, rails

# (interior sites, seeds per side, entries per row, link probability, one-way entries)
CASES = [(3, 1, 2, 0.5, False), (6, 2, 3, 0.4, True), (9, 3, 3, 0.35, False), (12, 4, 4, 0.3, True), (14, 5, 5, 0.3, False), (14, 5, 6, 0.45, True),
         (10, 2, 3, 0.25, False), (13, 4, 4, 0.5, False)]
TRIALS = 8


def _random_graph(rng, n_int, n_seed, nn, p, one_way):
    """n_seed seeds on either side round n_int other sites, some of them non-members; a seed is linked to few sites, so that W varies"""
    N = n_int + 2 * n_seed
    index = np.full((N, nn), -1, dtype=np.int32)
    for u in range(N):
        for e in range(nn):
            if rng.random() < p:
                v = int(rng.integers(0, N))
                far = (u < n_seed and v >= N - n_seed) or (v < n_seed and u >= N - n_seed)
                if v != u and not (far and rng.random() < 0.97):
                    index[u, e] = v
    if not one_way:                                                         # enter what fits in the other row too
        for u in range(N):
            for v in index[u][index[u] >= 0]:
                free = np.flatnonzero(index[v] < 0)
                if u not in index[v] and len(free):
                    index[v, free[0]] = u
    label = np.where(rng.random(N) < 0.9, rng.integers(0, N, N), rng.choice([-1, N, N + 7, -5], N)).astype(np.int32)
    return index, label, rng.normal(size=N)


def _check(res, index, label, x, nl, nr, max_strands=64):
    """the outputs against each other and against the graph; -> (C_L, C_R) as sorted arrays"""
    zone, strand, table, sites, info = res
    mask, ptr, nb, sl, sr = fl.graph(index, label, nl, nr)
    interior = mask & ~sl & ~sr
    assert np.array_equal(zone & fl.MEMBER, mask.astype(np.int32)) and (zone[~mask] == 0).all()
    assert info["interior"] == int(interior.sum())
    cl, cr_ = np.flatnonzero(zone & fl.LEFT_CUT), np.flatnonzero(zone & fl.RIGHT_CUT)
    W = info["width"]
    assert len(table["first_site"]) == max(W, 0) and (np.diff(table["first_site"]) > 0).all()
    if info["status"] in (2, 3):
        assert (zone[mask] == fl.MEMBER).all() and info["left_shore"] == info["right_shore"] == info["shared_cut"] == 0
    if info["status"] == 2:
        assert W == -1 and info["searches"] == info["rounds"] == 0 and (strand == -1).all() and len(sites) == 0
        return cl, cr_
    if info["status"] == 3:
        assert W == max_strands and info["searches"] == W
    else:
        assert info["status"] == (1 if W else 0) and info["searches"] == W + 2
        assert len(cl) == len(cr_) == W and interior[cl].all() and interior[cr_].all() and info["shared_cut"] == len(np.intersect1d(cl, cr_))
        for cut, bit, seeds, other in ((cl, fl.LEFT_SHORE, sl, sr), (cr_, fl.RIGHT_SHORE, sr, sl)):
            alive = mask.copy()
            alive[cut] = False
            hit, seen = fl.connected(ptr, nb, seeds, other, alive)
            assert not hit and np.array_equal((zone & bit) != 0, seen | seeds)
        assert info["left_shore"] == int(((zone & fl.LEFT_SHORE) != 0).sum()) and info["right_shore"] == int(((zone & fl.RIGHT_SHORE) != 0).sum())
        if x is not None and W:
            assert (info["cut_left_xmin"], info["cut_left_xmax"], info["cut_right_xmin"], info["cut_right_xmax"]) == \
                (x[cl].min(), x[cl].max(), x[cr_].min(), x[cr_].max())
        else:
            assert [info[k] for k in fl.X4] == [np.inf, -np.inf, np.inf, -np.inf]
    # the strands: valid, disjoint, W in number, each across each cut exactly once
    assert np.array_equal(table["offset"], np.cumsum(table["length"]) - table["length"]) and len(sites) == int(table["length"].sum())
    assert len(np.unique(sites)) == len(sites) and interior[sites].all()
    want = np.full(len(mask), -1, dtype=np.int32)
    for j in range(max(W, 0)):
        s = sites[table["offset"][j]:table["offset"][j] + table["length"][j]]
        want[s] = j
        assert len(s) >= 1 and s[0] == table["first_site"][j] and s[-1] == table["last_site"][j]
        assert all(b in nb[ptr[a]:ptr[a + 1]] for a, b in zip(s[:-1], s[1:]))
        left, right = nb[ptr[s[0]]:ptr[s[0] + 1]], nb[ptr[s[-1]]:ptr[s[-1] + 1]]
        assert table["left_seed"][j] == left[sl[left]].min() and table["right_seed"][j] == right[sr[right]].min()
        if info["status"] == 3:
            assert [table[k][j] for k in fl.STRANDS[6:]] == [-1] * 4
        else:
            a, b = np.flatnonzero(np.isin(s, cl)), np.flatnonzero(np.isin(s, cr_))
            assert len(a) == len(b) == 1 and a[0] <= b[0]
            assert [table[k][j] for k in fl.STRANDS[6:]] == [s[a[0]], a[0], s[b[0]], b[0]]
    assert np.array_equal(strand, want)
    assert (info["longest_strand"], info["shortest_strand"]) == ((table["length"].max(), table["length"].min()) if W > 0 else (0, 0))
    return cl, cr_


def _run_random(case):
    n_int, n_seed, nn, p, one_way = case
    rng = np.random.default_rng(hash(case[:3]) % 2 ** 32 + one_way)
    widths = []
    for trial in range(TRIALS):
        index, label, x = _random_graph(rng, n_int, n_seed, nn, p, one_way)
        x = None if trial == 0 else x
        res = fl.analyse(index, label, x, n_seed, n_seed)
        info = res[4]
        cl, cr_ = _check(res, index, label, x, n_seed, n_seed)
        assert info["interior"] <= 14
        W, minimum = fl.brute_width(index, label, n_seed, n_seed, all_minimum=True)           # the definition decides
        assert info["width"] == W and info["status"] == (2 if W < 0 else (1 if W else 0))
        widths.append(W)
        if W > 0:
            shore_l, shore_r = (res[0] & fl.LEFT_SHORE) != 0, (res[0] & fl.RIGHT_SHORE) != 0
            mask, ptr, nb, sl, sr = fl.graph(index, label, n_seed, n_seed)
            assert tuple(cl) in [m[0] for m in minimum] and tuple(cr_) in [m[0] for m in minimum]
            for sep, left in minimum:
                assert not (shore_l & ~left).any()                          # C_L's left shore lies inside every other one
                alive = mask.copy()
                alive[list(sep)] = False
                right = fl.connected(ptr, nb, sr, sl, alive)[1] | sr
                assert not (shore_r & ~right).any()
            # the stop at max_strands, at 1 and at W
            for cap in {1, W}:
                stopped = fl.analyse(index, label, x, n_seed, n_seed, max_strands=cap)
                assert stopped[4]["status"] == 3 and stopped[4]["width"] == cap
                _check(stopped, index, label, x, n_seed, n_seed, max_strands=cap)
    return widths


@pytest.mark.parametrize("case", CASES)
def test_flow_equals_brute_force(case):
    _run_random(case)


def test_random_graphs_reach_every_width():
    """W = 0 ... 4 and touching contacts all occur among the random graphs"""
    seen = set()
    for case in CASES:
        seen |= set(_run_random(case))
    print(sorted(seen))
    assert {-1, 0, 1, 2, 3, 4} <= seen


def test_against_networkx_on_larger_graphs():
    """in addition to the brute force: the value of the flow on the vertex-split graph"""
    nx = pytest.importorskip("networkx")
    rng = np.random.default_rng(11)
    for trial in range(12):
        n_int, n_seed = int(rng.integers(30, 120)), int(rng.integers(2, 9))
        index, label, x = _random_graph(rng, n_int, n_seed, int(rng.integers(2, 6)), 0.5, bool(trial % 2))
        res = fl.analyse(index, label, x, n_seed, n_seed)
        _check(res, index, label, x, n_seed, n_seed)
        mask, ptr, nb, sl, sr = fl.graph(index, label, n_seed, n_seed)
        g = nx.DiGraph()
        g.add_nodes_from(["s", "t"])
        node = lambda v, out: "s" if sl[v] else ("t" if sr[v] else (int(v), out))
        for v in np.flatnonzero(mask):
            if not sl[v] and not sr[v]:
                g.add_edge((int(v), 0), (int(v), 1), capacity=1)
            for w in nb[ptr[v]:ptr[v + 1]]:
                if node(v, 1) != node(w, 0) and not sr[v] and not sl[w]:
                    g.add_edge(node(v, 1), node(w, 0))                      # no capacity attribute: unbounded
        if res[4]["status"] == 2:
            continue
        assert res[4]["width"] == nx.maximum_flow_value(g, "s", "t")


# ---- hand cases ---------------------------------------------------------------------------------------------------------------------------
def _zone_sets(zone):
    return tuple(np.flatnonzero(zone & b).tolist() for b in (fl.LEFT_SHORE, fl.LEFT_CUT, fl.RIGHT_CUT, fl.RIGHT_SHORE))


def test_chain():
    n = 30
    x = np.arange(n) * 0.5
    index, label = _chain(n), np.zeros(n, dtype=np.int32)
    res = fl.analyse(index, label, x, 1, 1)
    zone, strand, table, sites, info = res
    _check(res, index, label, x, 1, 1)
    assert _zone_sets(zone) == ([0], [1], [n - 2], [n - 1])
    assert np.array_equal(sites, np.arange(1, n - 1)) and [int(table[k][0]) for k in fl.STRANDS] == [1, n - 2, n - 2, 0, 0, n - 1, 1, 0, n - 2, n - 3]
    # one search that finds the exit on level 2 (n - 2): levels + 1 rounds; two closing searches that label one in-node each: 2 rounds
    assert [info[k] for k in fl.INFO] == [1, 1, 1, 1, 0, n - 2, 1, 1, 3, 2 * (n - 2) + 1 + 2 + 2, n - 2, n - 2]
    assert [info[k] for k in fl.X4] == [0.5, 0.5, x[n - 2], x[n - 2]]
    assert fl.brute_width(index, label, 1, 1) == 1


def test_ladder():
    length = 12
    n = 2 * length
    index, label = index_of(ladder(length), n), np.zeros(n, dtype=np.int32)
    res = fl.analyse(index, label, None, 2, 2)
    _check(res, index, label, None, 2, 2)
    assert res[4]["width"] == 2 == fl.brute_width(index, label, 2, 2) and res[4]["status"] == 1
    assert _zone_sets(res[0]) == ([0, 1], [2, 3], [n - 4, n - 3], [n - 2, n - 1])


@pytest.mark.parametrize("k,length", [(3, 7), (6, 5)])
def test_rails_and_grid(k, length):
    n = k * length
    index, label = index_of(rails(k, length), n, nn=3), np.zeros(n, dtype=np.int32)
    res = fl.analyse(index, label, np.arange(n) * 1.0, k, k)
    _check(res, index, label, np.arange(n) * 1.0, k, k)
    assert res[4]["width"] == k and res[4]["longest_strand"] == res[4]["shortest_strand"] == length - 2
    assert _zone_sets(res[0])[1] == list(range(k, 2 * k)) and _zone_sets(res[0])[2] == list(range(n - 2 * k, n - k))


def test_shuffled_rails_cancel_flow():
    rng = np.random.default_rng(5)
    k, length = 6, 40
    n = k * length
    links = rails(k, length, rng) + [(int(rng.integers(k * i, k * i + k)), int(rng.integers(k * i + k, k * i + 2 * k))) for i in range(length - 1)]
    index, label = index_of(links, n, nn=6), np.zeros(n, dtype=np.int32)
    trace = {}
    res = fl.analyse(index, label, None, k, k, trace=trace)
    _check(res, index, label, None, k, k)
    assert res[4]["width"] == k and trace["backward"] >= 1


def test_two_ladders_joined_through_one_site():
    length = 5
    j = 2 * length
    n = 4 * length + 1
    links = ladder(length) + ladder(length, j + 1) + [(j - 2, j), (j - 1, j), (j, j + 1), (j, j + 2)]
    index, label = index_of(links, n), np.zeros(n, dtype=np.int32)
    res = fl.analyse(index, label, np.arange(n) * 1.0, 2, 2)
    _check(res, index, label, np.arange(n) * 1.0, 2, 2)
    assert res[4]["width"] == 1 and _zone_sets(res[0])[1] == [j] == _zone_sets(res[0])[2] and res[4]["shared_cut"] == 1
    assert [res[4][k] for k in fl.X4] == [float(j)] * 4


def test_contacts_that_touch():
    # a left seed linked to a right seed
    index, label = _chain(2), np.zeros(2, dtype=np.int32)
    res = fl.analyse(index, label, None, 1, 1)
    _check(res, index, label, None, 1, 1)
    assert [res[4][k] for k in fl.INFO] == [2, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0] and fl.brute_width(index, label, 1, 1) == -1
    # a member that is both a left and a right seed, beside a chain that does not touch
    index, label = _chain(5), np.zeros(5, dtype=np.int32)
    res = fl.analyse(index, label, None, 3, 3)
    _check(res, index, label, None, 3, 3)
    assert res[4]["status"] == 2 and res[4]["width"] == -1 and res[0].tolist() == [1] * 5
    # the same chain with that member taken out: nothing joins the contacts; four sites, two seeds a side: the seeds touch through a link
    label[2] = -1
    assert fl.analyse(index, label, None, 3, 3)[4]["status"] == 0
    assert fl.analyse(_chain(4), np.zeros(4, dtype=np.int32), None, 2, 2)[4]["status"] == 2


def test_empty_seed_set_and_no_sites():
    n = 6
    index, label = _chain(n), np.zeros(n, dtype=np.int32)
    res = fl.analyse(index, label, None, 0, 1)
    _check(res, index, label, None, 0, 1)
    # the right shore is everything the right seed reaches; one round per closing search on the left, n - 1 in-nodes deep on the right
    assert res[4]["status"] == 0 and res[4]["width"] == 0 and res[4]["left_shore"] == 0 and res[4]["right_shore"] == n and res[4]["searches"] == 2
    assert res[4]["rounds"] == 1 + (2 * (n - 1) + 1)
    res = fl.analyse(np.zeros((0, 3), dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0), 0, 0)
    assert [res[4][k] for k in fl.INFO] == [0] * 12 and len(res[0]) == len(res[1]) == len(res[3]) == 0
    # no member at all
    res = fl.analyse(index, np.full(n, -1, dtype=np.int32), None, 1, 1)
    assert res[4]["status"] == 0 and res[4]["searches"] == 2 and res[4]["rounds"] == 2 and (res[0] == 0).all()


def test_one_way_entries_link_both_ways():
    n = 7
    back = np.full((n, 1), -1, dtype=np.int32)
    back[1:, 0] = np.arange(n - 1)                                          # every link entered in the row of its right end only
    label = np.zeros(n, dtype=np.int32)
    a, b = fl.analyse(back, label, None, 1, 1), fl.analyse(_chain(n), label, None, 1, 1)
    fl.assert_equal(*a, b)
    assert a[4]["width"] == 1


# ---- the 2.5 nm golden device -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_2p5(cell_2p5):
    from devicekmc_amd import params, structure
    p = params.KMCParameters()
    el, neigh, nn, _ = structure.prepare_device(cell_2p5, p, None)
    return cell_2p5, p, el, neigh, nn


def test_pristine_2p5(device_2p5):
    s, p, el, neigh, nn = device_2p5
    nl, nr = _contacts(el, p.num_atoms_first_layer)
    label = np.where(cr.member_mask(el, None, list(p.metals), cr.METAL | cr.VACANCY_BIT), 0, -1).astype(np.int32)
    res = fl.analyse(neigh, label, s.x, nl, nr)
    _check(res, neigh, label, s.x, nl, nr)
    assert res[4]["status"] == 0 and res[4]["width"] == 0 and _zone_sets(res[0])[1] == [] == _zone_sets(res[0])[2]


@pytest.mark.parametrize("r", sorted(PINNED_2P5))
def test_pinned_planted_filaments_2p5(device_2p5, r):
    s, p, el, neigh, nn = device_2p5
    label, nl, nr, path = planted_2p5(s, p, el, neigh, r)
    res = fl.analyse(neigh, label, s.x, nl, nr)
    cl, cr_ = _check(res, neigh, label, s.x, nl, nr)
    info = res[4]
    print(r, info, cl.tolist(), cr_.tolist(), {k: v.tolist() for k, v in res[2].items()})
    assert (info["width"], cl.tolist(), cr_.tolist()) == PINNED_2P5[r]
    assert (info["searches"], info["rounds"]) == PINNED_2P5_ROUNDS[r]
    if info["width"] == 1:
        # the cut sites of the canonical path that are no seeds: C_L is the first of them, C_R the last
        table = cu.analyse(neigh, label, s.x, nl, nr, path)[2]
        cuts = [v for v in table["site"][table["cut"] == 1] if nl <= v < len(label) - nr]
        assert cl.tolist() == [cuts[0]] and cr_.tolist() == [cuts[-1]]
        assert cl[0] == path[12]
