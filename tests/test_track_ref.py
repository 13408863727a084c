"""The host reference of the cluster tracking (track_ref.py) checked on its own: analyse() against brute() on random label pairs, hand cases in
which every flag, every change code and every transition occurs and is asserted by name, and the pinned figures of the planted filaments on the
2.5 nm device.  No GPU."""
import numpy as np
import pytest

import cluster_ref as cr
import track_ref as tr
from analysis_support import _contacts
from track_ref import PINNED_2P5, PINNED_MEMBERS, PLANTINGS, _rows, check_pinned_2p5, random_pair  # noqa: F401


@pytest.mark.parametrize("N", [1, 2, 7, 64, 65, 300])
def test_reference_equals_brute_force(N):
    rng = np.random.default_rng(100 + N)
    seen = set()
    for k_prev in (1, 2, 5, N):
        for k_now in (1, 2, 5, N):
            for p in (0.3, 0.9):
                lp, ln, x = random_pair(rng, N, k_prev, k_now, p)
                nl, nr = int(rng.integers(0, N + 1)) // 3, int(rng.integers(0, N + 1)) // 3
                ref = tr.analyse(lp, ln, x, nl, nr)
                tr.assert_equal(*tr.brute(lp, ln, x, nl, nr), ref)
                change, pairs, now, prev, critical, info = ref
                # sums that tie the tables together
                assert pairs["count"].sum() == (change != 0).sum() == info["stayed"] + info["joined"] + info["left"]
                assert now["size"].sum() == info["stayed"] + info["joined"] and prev["size"].sum() == info["stayed"] + info["left"]
                assert now["joined"].sum() == info["joined"] and prev["left"].sum() == info["left"]
                assert now["n_parents"].sum() == prev["n_children"].sum() == int(((pairs["prev"] >= 0) & (pairs["now"] >= 0)).sum())
                assert (np.diff(pairs["first_site"]) > 0).all() and (np.diff(now["root"]) > 0).all() and (np.diff(prev["root"]) > 0).all()
                seen.add(info["transition"])
    assert N < 64 or seen == {0, 1, 2, 3}
    # x missing: the same result but for the range
    ref = tr.analyse(lp, ln, None, nl, nr)
    tr.assert_equal(*tr.brute(lp, ln, None, nl, nr), ref)
    assert ref[5]["critical_xmin"] == np.inf and ref[5]["critical_xmax"] == -np.inf


def test_empty_inputs():
    e = np.zeros(0, dtype=np.int32)
    for ref in (tr.analyse(e, e, np.zeros(0), 3, 3), tr.analyse(np.full(9, -1), np.full(9, 9), np.zeros(9), 3, 3)):
        change, pairs, now, prev, critical, info = ref
        assert all(info[k] == (-1 if k.startswith("bridge") else 0) for k in tr.INFO) and info["critical_xmin"] == np.inf
        assert len(pairs["prev"]) == len(now["root"]) == len(prev["root"]) == len(critical) == 0 and not change.any()


def test_hand_case_every_flag_and_code():
    #                 0  1  2  3  4   5  6  7   8   9  10  11  12  13
    prev = np.array([0, 0, 0, 3, 3, -1, 6, 6,  8, -1, -1, 11, 11, 11], dtype=np.int32)
    now = np.array([0, 0, 0, 0, 0,  0, 6, 7, -1,  9, 99, 11, 11, 11], dtype=np.int32)
    ref = tr.analyse(prev, now, np.arange(14) * 0.5, 2, 2)
    tr.assert_equal(*tr.brute(prev, now, np.arange(14) * 0.5, 2, 2), ref)
    change, pairs, n, p, critical, info = ref
    assert change.tolist() == [tr.STAYED] * 3 + [tr.REGROUPED] * 2 + [tr.JOINED, tr.STAYED, tr.REGROUPED, tr.LEFT_, tr.JOINED, tr.NONE] + [tr.STAYED] * 3
    assert [pairs[k].tolist() for k in tr.PAIRS] == [[0, 3, -1, 6, 6, 8, -1, 11], [0, 0, 0, 6, 7, -1, 9, 11], [3, 2, 1, 1, 1, 1, 1, 3], [0, 3, 5, 6, 7, 8, 9, 11]]
    # now table: 0 merged from 0 and 3 (+ one joiner), 6 and 7 the fragments of 6, 9 born
    assert _rows(n, 0) == dict(root=0, size=6, joined=1, n_parents=2, main_parent=0, flags=tr.TOUCH_LEFT | tr.MERGED)
    assert _rows(n, 6) == dict(root=6, size=1, joined=0, n_parents=1, main_parent=6, flags=tr.FRAGMENT)
    assert _rows(n, 7) == dict(root=7, size=1, joined=0, n_parents=1, main_parent=6, flags=tr.FRAGMENT)
    assert _rows(n, 9) == dict(root=9, size=1, joined=1, n_parents=0, main_parent=-1, flags=tr.BORN)
    assert _rows(n, 11) == dict(root=11, size=3, joined=0, n_parents=1, main_parent=11, flags=tr.TOUCH_RIGHT)
    # prev table: 0 and 3 absorbed into the merged 0, 6 split (its main child the smaller id on the tie 1 : 1), 8 died
    assert _rows(p, 0) == dict(root=0, size=3, left=0, n_children=1, main_child=0, flags=tr.TOUCH_LEFT | tr.ABSORBED)
    assert _rows(p, 3) == dict(root=3, size=2, left=0, n_children=1, main_child=0, flags=tr.ABSORBED)
    assert _rows(p, 6) == dict(root=6, size=2, left=0, n_children=2, main_child=6, flags=tr.SPLIT)
    assert _rows(p, 8) == dict(root=8, size=1, left=1, n_children=0, main_child=-1, flags=tr.DIED)
    assert _rows(p, 11) == dict(root=11, size=3, left=0, n_children=1, main_child=11, flags=tr.TOUCH_RIGHT)
    assert info == dict(n_prev=5, n_now=5, n_pairs=8, stayed=10, joined=2, left=1, regrouped=3, transition=tr.OPEN, bridge_prev=-1, bridge_now=-1,
                        born=1, died=1, merged=1, split=1, n_critical=0, critical_xmin=np.inf, critical_xmax=-np.inf)
    assert len(critical) == 0


def test_main_parent_tie_goes_to_the_smaller_id():
    now = np.zeros(4, dtype=np.int32)
    for prev, want in (([0, 0, 2, 2], 0), ([3, 3, 1, 1], 1), ([2, 1, 1, 2], 1)):
        ref = tr.analyse(np.array(prev, dtype=np.int32), now, None, 0, 0)
        tr.assert_equal(*tr.brute(np.array(prev, dtype=np.int32), now, None, 0, 0), ref)
        assert _rows(ref[2], 0)["main_parent"] == want and _rows(ref[2], 0)["n_parents"] == 2
        # the sites of the main parent stayed on the main line, the others regrouped
        assert ref[0].tolist() == [tr.STAYED if v == want else tr.REGROUPED for v in prev]
    # the larger count wins over the smaller id
    ref = tr.analyse(np.array([4, 4, 4, 1, 1], dtype=np.int32), np.zeros(5, dtype=np.int32), None, 0, 0)
    assert _rows(ref[2], 0)["main_parent"] == 4


def test_transitions_and_critical_sites():
    x = np.array([0.0, 1.0, 2.5, 2.0, 4.0, 5.0])
    tips = np.array([0, 0, -1, -1, 4, 4], dtype=np.int32)
    full = np.zeros(6, dtype=np.int32)
    # closed: the two sites whose arrival joined the tips
    change, pairs, now, prev, critical, info = tr.analyse(tips, full, x, 1, 1)
    assert (info["transition"], info["bridge_prev"], info["bridge_now"]) == (tr.CLOSED, -1, 0)
    assert critical.tolist() == [2, 3] and (info["critical_xmin"], info["critical_xmax"]) == (2.0, 2.5)
    assert _rows(now, 0)["flags"] == tr.TOUCH_LEFT | tr.TOUCH_RIGHT | tr.MERGED and info["merged"] == 1
    # ruptured: the same two sites, lost
    change, pairs, now, prev, critical, info = tr.analyse(full, tips, x, 1, 1)
    assert (info["transition"], info["bridge_prev"], info["bridge_now"]) == (tr.RUPTURED, 0, -1)
    assert critical.tolist() == [2, 3] and (info["critical_xmin"], info["critical_xmax"]) == (2.0, 2.5)
    assert _rows(prev, 0)["flags"] == tr.TOUCH_LEFT | tr.TOUCH_RIGHT | tr.SPLIT and info["split"] == 1
    assert change.tolist() == [tr.STAYED, tr.STAYED, tr.LEFT_, tr.LEFT_, tr.REGROUPED, tr.REGROUPED]
    # bridged -> bridged and open -> open: no critical site
    for lab, t in ((full, tr.BRIDGED), (tips, tr.OPEN)):
        change, _, _, _, critical, info = tr.analyse(lab, lab, x, 1, 1)
        assert info["transition"] == t and len(critical) == 0 and info["critical_xmin"] == np.inf and info["regrouped"] == 0
    # a joiner of another cluster is not critical
    change, _, _, _, critical, info = tr.analyse(np.array([0, -1, -1, 3, -1, 5], dtype=np.int32), np.array([0, 0, 0, 0, 4, 0], dtype=np.int32), x, 1, 1)
    assert info["transition"] == tr.CLOSED and critical.tolist() == [1, 2] and change[4] == tr.JOINED and info["born"] == 1


@pytest.fixture(scope="module")
def labels_2p5(cell_2p5):
    from devicekmc_amd import params, structure
    p = params.KMCParameters()
    el, neigh, nn, _ = structure.prepare_device(cell_2p5, p, None)
    nl, nr = _contacts(el, p.num_atoms_first_layer)
    labels = {}
    for name, planting in PLANTINGS.items():
        el2 = el if planting is None else cr.plant_filament(el, cell_2p5.x, cell_2p5.y, cell_2p5.z, *planting)[0]
        labels[name], _, info = cr.analyse(neigh, el2, None, cell_2p5.x, list(p.metals), cr.METAL | cr.VACANCY_BIT, nl, nr, with_rounds=False)
        assert info["n_members"] == PINNED_MEMBERS[name]
    return labels, cell_2p5.x, nl, nr


@pytest.mark.parametrize("key", list(PINNED_2P5))
def test_pinned_figures_2p5(labels_2p5, key):
    labels, x, nl, nr = labels_2p5
    ref = tr.analyse(labels[key[0]], labels[key[1]], x, nl, nr)
    tr.assert_equal(*tr.brute(labels[key[0]], labels[key[1]], x, nl, nr), ref)     # confirmed by the brute force, then pinned
    check_pinned_2p5(key, ref)


def test_closing_and_rupture_name_the_same_sites(labels_2p5):
    labels, x, nl, nr = labels_2p5
    closed, ruptured = tr.analyse(labels["open"], labels["full"], x, nl, nr), tr.analyse(labels["full"], labels["open"], x, nl, nr)
    assert len(closed[4]) == 25 and np.array_equal(closed[4], ruptured[4])
    assert np.array_equal(np.flatnonzero(closed[0] == tr.JOINED), closed[4]) and np.array_equal(np.flatnonzero(ruptured[0] == tr.LEFT_), closed[4])
