"""The host reference of the cut-site analysis (cut_ref.py) checked on its own: the rule of the off-path components and chords against the
definition (delete a member, search) on small random graphs, its independence of the path used, hand cases, and the planted filaments of the
2.5 nm golden device, whose figures are pinned here.  No GPU."""
import numpy as np
import pytest

import cluster_ref as cr
import cut_ref as cu
import path_ref as pr
from analysis_support import _random_case, index_of, ladder
from analysis_support import ordered_chain as _chain
from cut_ref import PINNED_2P5, PINNED_2P5_WIDE_BYPASS, planted_2p5

CASES = [(1, 1, 1.0, 0.0), (7, 2, 0.8, 0.3), (40, 3, 0.5, 0.5), (63, 2, 0.9, 0.2), (150, 4, 0.3, 0.1)]
TRIALS = 6


def _seeds(N):
    """two fifths of the sites on either side (at least one): most of the random graphs are connected then"""
    return max(1, (2 * N) // 5), max(1, (2 * N) // 5)


def _random_graph(rng, N, nn, p_member, p_pad, one_way):
    index, element, _, x = _random_case(rng, N, nn, p_member, p_pad, one_way)
    label = np.where(element != 3, rng.integers(0, N, N), rng.choice([-1, N, N + 7, -5], N)).astype(np.int32)
    return index, label, x


def _cut_set(res):
    table = res[2]
    return np.sort(table["site"][table["cut"] == 1])


def _check_tables(res, x):
    """the columns against each other and against info"""
    role, bypass, table, byp, necks, info = res
    L = len(table["site"])
    assert np.array_equal(table["cut"], ((table["n_bypass"] == 0) & (table["chord"] == 0)).astype(np.int32))
    assert info["cut_sites"] == int(table["cut"].sum()) == int((role == cu.CUT).sum()) and int((role == cu.PATH_SITE).sum()) == L - info["cut_sites"]
    assert info["path_len"] == L and info["max_bypass"] == (int(table["n_bypass"].max()) if L else 0)
    assert info["chord_positions"] == int(table["chord"].sum()) and info["bypasses"] == len(byp["root"])
    assert (np.diff(byp["root"]) > 0).all() and (byp["hi"] - byp["lo"] >= 2).all()
    off = bypass >= 0
    assert info["offpath_members"] == int(off.sum()) and info["offpath_components"] == len(np.unique(bypass[off]))
    assert np.array_equal(off, role >= cu.BYPASS) and (bypass[table["site"]] == -1).all()
    for j, r in enumerate(byp["root"]):
        assert byp["size"][j] == int((bypass == r).sum()) and (role[bypass == r] == cu.BYPASS).all() and -1 <= byp["lo"][j] < byp["hi"][j] <= L
    assert int((role == cu.BYPASS).sum()) == int(byp["size"].sum())
    cover = np.zeros(L, dtype=np.int64)
    for lo, hi in zip(byp["lo"], byp["hi"]):
        cover[lo + 1:hi] += 1
    assert np.array_equal(cover, table["n_bypass"])
    # necks: the runs of cut positions
    assert info["necks"] == len(necks["first"]) and int((necks["last"] - necks["first"] + 1).sum()) == info["cut_sites"]
    for j in range(info["necks"]):
        a, b = necks["first"][j], necks["last"][j]
        assert table["cut"][a:b + 1].all() and (a == 0 or not table["cut"][a - 1]) and (b == L - 1 or not table["cut"][b + 1])
        if x is not None:
            assert necks["xmin"][j] == x[table["site"][a:b + 1]].min() and necks["xmax"][j] == x[table["site"][a:b + 1]].max()
    if info["necks"]:
        length = necks["last"] - necks["first"] + 1
        assert info["longest_neck"] == length.max() and info["longest_neck_first"] == necks["first"][np.argmax(length)]
    else:
        assert (info["longest_neck"], info["longest_neck_first"]) == (0, -1)


@pytest.mark.parametrize("one_way", [False, True])
@pytest.mark.parametrize("N,nn,p_member,p_pad", CASES)
def test_rule_equals_brute_force_and_does_not_depend_on_the_path(N, nn, p_member, p_pad, one_way):
    """returns nothing; the counts over all cases are asserted in test_random_graphs_cover_the_cases"""
    _run_random(N, nn, p_member, p_pad, one_way)


def _run_random(N, nn, p_member, p_pad, one_way):
    rng = np.random.default_rng(1000 * N + nn + one_way)
    nl, nr = _seeds(N)
    connected = longer = chords = 0
    for trial in range(TRIALS):
        index, label, x = _random_graph(rng, N, nn, p_member, p_pad, one_way)
        canon = pr.analyse(index, label, x, nl, nr, 0)[2]
        mask, ptr, nb, sl, sr = cu.graph(index, label, nl, nr)
        res0 = cu.analyse(index, label, x, nl, nr, np.zeros(0, dtype=np.int32))
        _check_tables(res0, x)
        assert res0[5]["status"] == 0 and (res0[0][mask] == cu.APART).all() and (res0[0][~mask] == 0).all() and res0[5]["bypasses"] == 0
        if len(canon) == 0:
            continue
        connected += 1
        brute = cu.brute_cut_set(index, label, nl, nr)
        res = cu.analyse(index, label, x, nl, nr, canon)
        _check_tables(res, x)
        assert res[5]["status"] == 1 and np.array_equal(_cut_set(res), brute)
        # every cut site lies on every path: the members off the path are no cut sites
        assert np.isin(brute, canon).all()
        for _ in range(2):
            path = cu.random_simple_path(rng, ptr, nb, sl, sr)
            assert len(path) >= len(canon) and cu.check_path(path, N, mask, ptr, nb, sl, sr) is None
            other = cu.analyse(index, label, None, nl, nr, path)
            _check_tables(other, None)
            assert np.array_equal(_cut_set(other), brute)
            longer += len(path) > len(canon)
            chords += int(other[5]["chord_positions"] > 0)
    return connected, longer, chords


def test_random_graphs_cover_the_cases():
    """at least half of the random graphs are connected; some of the random paths are longer than the shortest one, some carry chords"""
    tot = np.zeros(3, dtype=np.int64)
    n = 0
    for case in CASES:
        for one_way in (False, True):
            tot += _run_random(*case, one_way)
            n += TRIALS
    print(n, tot)
    assert 2 * tot[0] >= n and tot[1] > 0 and tot[2] > 0


def test_invalid_paths_are_named():
    n = 6
    chain = _chain(n)
    label = np.array([0, 0, 0, 0, -1, 0], dtype=np.int32)
    good = cu.analyse(chain, np.zeros(n, dtype=np.int32), None, 1, 1, np.arange(n))
    assert good[5]["cut_sites"] == n
    for path, row in (([0, 1, 1, 2], 2), ([0, 2], 1), ([1, 2], 0), ([0, 1, 2, 3, 4, 5], 4), ([0, 1, 2], 2), ([0, 7], 1)):
        with pytest.raises(ValueError, match="row %d" % row):
            cu.analyse(chain, label if 4 in path else np.zeros(n, dtype=np.int32), None, 1, 1, np.array(path))


# ---- hand cases ---------------------------------------------------------------------------------------------------------------------------
def test_ordered_chain_is_one_neck():
    n = 30
    x = np.arange(n) * 0.5
    role, bypass, table, byp, necks, info = cu.analyse(_chain(n), np.zeros(n, dtype=np.int32), x, 1, 1, np.arange(n))
    assert (role == cu.CUT).all() and (bypass == -1).all() and table["cut"].all() and len(byp["root"]) == 0
    assert (necks["first"].tolist(), necks["last"].tolist(), necks["xmin"].tolist(), necks["xmax"].tolist()) == ([0], [n - 1], [0.0], [x[-1]])
    assert [info[k] for k in cu.INFO] == [1, n, n, 1, n, 0, 0, 0, 0, 0, 0, 1]
    assert np.array_equal(cu.brute_cut_set(_chain(n), np.zeros(n, dtype=np.int32), 1, 1), np.arange(n))
    # without x the necks hold +inf / -inf
    necks = cu.analyse(_chain(n), np.zeros(n, dtype=np.int32), None, 1, 1, np.arange(n))[4]
    assert np.isposinf(necks["xmin"]).all() and np.isneginf(necks["xmax"]).all()


def test_ladder_has_no_cut_site():
    length = 12
    n = 2 * length
    index, label = index_of(ladder(length), n), np.zeros(n, dtype=np.int32)
    path = pr.analyse(index, label, None, 2, 2, 0)[2]
    role, bypass, table, byp, necks, info = cu.analyse(index, label, None, 2, 2, path)
    assert np.array_equal(path, 2 * np.arange(length)) and info["cut_sites"] == 0 and info["necks"] == 0 and len(necks["first"]) == 0
    assert (byp["root"].tolist(), byp["size"].tolist(), byp["lo"].tolist(), byp["hi"].tolist()) == ([1], [length], [-1], [length])
    assert (table["n_bypass"] == 1).all() and (table["chord"] == 0).all() and (role[1::2] == cu.BYPASS).all() and (bypass[1::2] == 1).all()
    assert len(cu.brute_cut_set(index, label, 2, 2)) == 0


def test_two_ladders_joined_through_one_site():
    length = 5
    j = 2 * length                                                          # the joint
    n = 4 * length + 1
    links = ladder(length) + ladder(length, j + 1) + [(j - 2, j), (j - 1, j), (j, j + 1), (j, j + 2)]
    index, label = index_of(links, n), np.zeros(n, dtype=np.int32)
    path = pr.analyse(index, label, None, 2, 2, 0)[2]
    role, bypass, table, byp, necks, info = cu.analyse(index, label, np.arange(n) * 1.0, 2, 2, path)
    assert _cut_set((role, bypass, table, byp, necks, info)).tolist() == [j] == cu.brute_cut_set(index, label, 2, 2).tolist()
    assert info["necks"] == 1 and necks["first"][0] == necks["last"][0] == length and necks["xmin"][0] == necks["xmax"][0] == float(j)
    assert info["bypasses"] == 2 and byp["lo"].tolist() == [-1, length] and byp["hi"].tolist() == [length, 2 * length + 1]


def test_one_site_that_is_both_seeds():
    index = np.array([[-1]], dtype=np.int32)
    res = cu.analyse(index, np.zeros(1, dtype=np.int32), None, 1, 1, [0])
    assert res[0].tolist() == [cu.CUT] and [res[5][k] for k in cu.INFO] == [1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1]
    assert cu.brute_cut_set(index, np.zeros(1, dtype=np.int32), 1, 1).tolist() == [0]
    # a second such site beside it: either one alone still connects the contacts
    index = np.array([[1], [-1]], dtype=np.int32)
    res = cu.analyse(index, np.zeros(2, dtype=np.int32), None, 2, 2, [0])
    assert res[0].tolist() == [cu.PATH_SITE, cu.BYPASS] and res[2]["n_bypass"].tolist() == [1] and res[5]["cut_sites"] == 0
    assert (res[3]["lo"].tolist(), res[3]["hi"].tolist()) == ([-1], [1])
    assert len(cu.brute_cut_set(index, np.zeros(2, dtype=np.int32), 2, 2)) == 0


def test_empty_inputs():
    res = cu.analyse(np.zeros((0, 3), dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0), 0, 0, [])
    assert [res[5][k] for k in cu.INFO] == [0, 0, 0, 0, 0, -1, 0, 0, 0, 0, 0, 0] and len(res[0]) == len(res[1]) == 0
    res = cu.analyse(np.array([[1], [0]], dtype=np.int32), np.array([-1, 2], dtype=np.int32), None, 1, 1, [])
    assert res[0].tolist() == [0, 0] and res[1].tolist() == [-1, -1] and res[5]["rounds"] == 1 and res[5]["offpath_members"] == 0


# ---- the 2.5 nm golden device -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_2p5(cell_2p5):
    from devicekmc_amd import params, structure
    p = params.KMCParameters()
    el, neigh, nn, _ = structure.prepare_device(cell_2p5, p, None)
    return cell_2p5, p, el, neigh, nn


@pytest.mark.parametrize("r", [3.0, 2.6, 2.4, 2.2])
def test_pinned_planted_filaments_2p5(device_2p5, r):
    s, p, el, neigh, nn = device_2p5
    label, nl, nr, path = planted_2p5(s, p, el, neigh, r)
    res = cu.analyse(neigh, label, s.x, nl, nr, path)
    _check_tables(res, s.x)
    role, bypass, table, byp, necks, info = res
    print(r, info, np.flatnonzero(table["cut"]).tolist(), {k: v.tolist() for k, v in byp.items()}, {k: v.tolist() for k, v in necks.items()})
    assert np.array_equal(_cut_set(res), cu.brute_cut_set(neigh, label, nl, nr, sites=path))           # the definition decides
    assert (info["path_len"], np.flatnonzero(table["cut"]).tolist(), info["necks"], info["longest_neck"], info["longest_neck_first"],
            info["bypasses"]) == PINNED_2P5[r]
    if r == 3.0:
        assert tuple(int(byp[k][0]) for k in cu.BYPASSES) == PINNED_2P5_WIDE_BYPASS
