"""The host reference of the filament analysis (cluster_ref.py) checked on its own: against a brute-force flood fill on small random graphs,
against the pinned component counts of the two golden devices and on the planted filaments.  No GPU."""
import numpy as np
import pytest

import cluster_ref as cr
from analysis_support import _contacts, _random_case
from conftest import params_7p5

METALS = [4, 5, 6, 7, 8]


@pytest.mark.parametrize("one_way", [False, True])
@pytest.mark.parametrize("N,nn,p_member,p_pad", [(1, 1, 1.0, 0.0), (7, 2, 0.8, 0.3), (40, 3, 0.5, 0.5), (63, 2, 0.9, 0.2), (150, 4, 0.3, 0.1)])
def test_reference_equals_flood_fill(N, nn, p_member, p_pad, one_way):
    rng = np.random.default_rng(1000 * N + nn + one_way)
    for members in (cr.METAL | cr.VACANCY_BIT, cr.VACANCY_BIT, cr.VACANCY_BIT | cr.NEUTRAL_ONLY, cr.METAL):
        index, element, charge, x = _random_case(rng, N, nn, p_member, p_pad, one_way)
        label, table, info = cr.analyse(index, element, charge, x, [6], members, N // 4, N // 4)
        mask = cr.member_mask(element, charge, [6], members)
        brute = cr.flood_fill(index, mask)
        assert np.array_equal(label, brute)
        # the table from the brute-force labels, row by row
        roots = np.unique(brute[brute >= 0])
        assert np.array_equal(table["root"], roots) and info["n_components"] == len(roots) and info["n_members"] == int(mask.sum())
        for j, r in enumerate(roots):
            ids = np.flatnonzero(brute == r)
            assert table["size"][j] == len(ids) and table["n_vacancy"][j] == int((element[ids] == 2).sum())
            assert table["flags"][j] == (1 if (ids < N // 4).any() else 0) + (2 if (ids >= N - N // 4).any() else 0)
            assert table["xmin"][j] == x[ids].min() and table["xmax"][j] == x[ids].max()
        both = table["flags"] == 3
        assert info["bridged"] == int(both.any()) and info["bridge_root"] == (roots[both][0] if both.any() else -1)
        assert (info["gap_x"] == 0.0) if info["bridged"] else (info["gap_x"] == info["tip_right_x"] - info["tip_left_x"])
        assert 1 <= info["rounds"] <= 64


def test_neutral_only_drops_the_charged_vacancies():
    index = np.array([[1], [2], [-1]], dtype=np.int32)
    element = np.array([2, 2, 2], dtype=np.int32)
    label, _, info = cr.analyse(index, element, np.array([0, 2, 0]), np.zeros(3), METALS, cr.VACANCY_BIT | cr.NEUTRAL_ONLY, 0, 0)
    assert label.tolist() == [0, -1, 2] and info["n_components"] == 2
    label, _, _ = cr.analyse(index, element, np.array([0, 2, 0]), np.zeros(3), METALS, cr.VACANCY_BIT, 0, 0)
    assert label.tolist() == [0, 0, 0]


def test_model_rounds_of_chains():
    """the synchronous model: an ordered chain closes in two rounds (hook everything, then see nothing left); a randomly numbered chain of
    20 000 sites stays far below the cap of 64"""
    n = 20000
    chain = np.stack([np.arange(n) - 1, np.r_[np.arange(1, n), -1]], axis=1).astype(np.int32)
    assert cr.model_rounds(chain, np.ones(n, dtype=bool))[0] == 2
    perm = np.random.default_rng(3).permutation(n)
    scr = np.full((n, 2), -1, dtype=np.int32)
    scr[perm[:-1], 0] = perm[1:]; scr[perm[1:], 1] = perm[:-1]
    rounds, root = cr.model_rounds(scr, np.ones(n, dtype=bool))
    assert not root.any() and 3 <= rounds <= 16


@pytest.fixture(scope="module")
def device_2p5(cell_2p5):
    from devicekmc_amd import params, structure
    p = params.KMCParameters()
    el, neigh, nn, _ = structure.prepare_device(cell_2p5, p, None)
    return cell_2p5, p, el, neigh, nn


def test_pinned_counts_2p5(device_2p5):
    s, p, el, neigh, nn = device_2p5
    assert (len(el), nn) == (9399, 51)
    nl, nr = _contacts(el, p.num_atoms_first_layer)
    _, table, info = cr.analyse(neigh, el, None, s.x, list(p.metals), cr.METAL | cr.VACANCY_BIT, nl, nr)
    assert (info["n_members"], info["n_components"]) == (3521, 79)
    assert int((table["size"] == 1).sum()) == 66 and sorted(table["size"])[-2:] == [1449, 1982]
    _, _, info = cr.analyse(neigh, el, None, s.x, list(p.metals), cr.VACANCY_BIT, nl, nr)
    assert (info["n_members"], info["n_components"]) == (100, 83)


def test_pinned_counts_7p5(dev_7p5):
    from devicekmc_amd import structure
    p = params_7p5()
    el, neigh, nn, _ = structure.prepare_device(dev_7p5, p, None)
    assert (len(el), nn) == (85071, 52)
    nl, nr = _contacts(el, p.num_atoms_first_layer)
    _, table, info = cr.analyse(neigh, el, None, dev_7p5.x, list(p.metals), cr.METAL | cr.VACANCY_BIT, nl, nr)
    assert (info["n_members"], info["n_components"]) == (31681, 629)
    assert sorted(table["size"])[-2:] == [12994, 17862]
    assert info["rounds"] <= 8
    _, _, info = cr.analyse(neigh, el, None, dev_7p5.x, list(p.metals), cr.VACANCY_BIT, nl, nr, with_rounds=False)
    assert (info["n_members"], info["n_components"]) == (900, 691)


@pytest.mark.parametrize("r,skip,planted,components,bridged", [(3.0, None, 85, 65, 1), (3.0, (25.0, 40.0), 60, 70, 0), (2.0, None, 36, 73, 0)])
def test_planted_filament_2p5(device_2p5, r, skip, planted, components, bridged):
    s, p, el, neigh, nn = device_2p5
    el2, n = cr.plant_filament(el, s.x, s.y, s.z, r, skip)
    assert n == planted
    nl, nr = _contacts(el2, p.num_atoms_first_layer)
    _, _, info = cr.analyse(neigh, el2, None, s.x, list(p.metals), cr.METAL | cr.VACANCY_BIT, nl, nr)
    assert info["n_components"] == components and info["bridged"] == bridged
    if bridged:
        assert info["bridge_root"] == 0 and info["gap_x"] == 0.0
    elif skip:
        assert abs(info["tip_left_x"] - 24.18) <= 0.005 and abs(info["tip_right_x"] - 38.57) <= 0.005 and abs(info["gap_x"] - 14.4) <= 0.05
    else:
        assert abs(info["gap_x"] - 3.86) <= 0.005      # the printed digits of the pinned figures
