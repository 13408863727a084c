"""The one labelling body (csrc/rounds.h: k_lab_hook, k_lab_compress, label_rounds) under both of its callers: dkmc_find_clusters, and
dkmc_find_cuts on those labels with an empty path -- every member is off the path then, so the cut analysis labels the same member set over the
same index and has to end on the same roots after the same number of rounds, the number of the host model (cluster_ref.model_rounds)."""
import numpy as np
import pytest

import cluster_ref as cr
from analysis_support import _chain, _dev, hip  # noqa: F401

pytestmark = pytest.mark.gpu

VACANCY, OXYGEN = 2, 3                            # a member / a non-member with members = VACANCY_BIT
ROUND_BATCH = 8                                   # rounds the driver enqueues per read-back (csrc/rounds.h)


@pytest.fixture(autouse=True)
def _default_caps(hip):
    yield
    hip[1].dkmc_debug_set_cluster_round_cap(0)
    hip[1].dkmc_debug_set_cut_round_cap(0)


def _both(hip, index, mask):
    """find_clusters on the members of mask, find_cuts on its labels with an empty path; the checks every case shares -> rounds"""
    host, _ = hip
    N, nn = index.shape
    d_index = _dev(index, np.int32)
    label, _, cl = host.find_clusters(d_index, nn, _dev(np.where(mask, VACANCY, OXYGEN), np.int32), None, _dev(np.zeros(N), np.float64),
                                      _dev([6], np.int32), cr.VACANCY_BIT, N // 5, N // 3)
    _, bypass, _, _, _, cu = host.find_cuts(d_index, nn, label, None, N // 5, N // 3, None)
    assert bypass.cpu().numpy().tobytes() == label.cpu().numpy().tobytes()
    rounds, root = cr.model_rounds(index, mask)
    print("N %d nn %d: rounds clusters %d cuts %d model %d" % (N, nn, cl["rounds"], cu["rounds"], rounds))
    assert np.array_equal(label.cpu().numpy(), root)
    assert cu["rounds"] == cl["rounds"] == rounds
    assert cu["offpath_components"] == cl["n_components"] and cu["offpath_members"] == cl["n_members"] == int(mask.sum())
    return rounds


@pytest.mark.parametrize("one_way", [False, True], ids=["both-ways", "one-way"])
@pytest.mark.parametrize("N,nn", [(1, 1), (63, 2), (65, 3), (257, 2), (300, 130)])
def test_random_graphs(hip, N, nn, one_way):
    """the wave and workgroup edges, and 16 lanes and the whole wave per row; padding anywhere in a row and past the end"""
    rng = np.random.default_rng(13 * N + nn + one_way)
    index = rng.integers(0, N, size=(N, nn)).astype(np.int32)
    index[rng.random((N, nn)) < (0.985 if nn == 130 else 0.4)] = -1
    index[rng.random((N, nn)) < 0.02] = N + 3
    if one_way:
        index[(index >= 0) & (index < np.arange(N)[:, None])] = -1
    _both(hip, index, rng.random(N) < 0.7)


def _scrambled_chains(n=200):
    """Two numberings of a chain of n sites.  random: a permutation; its labelling takes 6 or 7 rounds at n = 200, inside one batch.  ruler: the
    position with more trailing zero bits gets the smaller site index, so the roots along the chain alternate between a local minimum and a site
    that hooks under one: every round halves the components and no round does more -- a round cannot do less, since every root with a smaller
    neighbouring root is hooked --, ceil(log2 n) + 1 = 9 rounds at n = 200, the most a graph of 200 sites can take: the last one is read back
    with the second batch."""
    pos = np.arange(n)
    tz = np.array([64 if p == 0 else (p & -p).bit_length() - 1 for p in range(n)])
    ruler = np.empty(n, dtype=np.int64)
    ruler[np.lexsort((pos, -tz))] = pos                                            # site index of position p
    return {"random": np.random.default_rng(3).permutation(n), "ruler": ruler}


@pytest.mark.parametrize("numbering", ["random", "ruler"])
def test_scrambled_chain(hip, numbering):
    order = _scrambled_chains()[numbering]
    rounds = _both(hip, _chain(order), np.ones(len(order), dtype=bool))
    if numbering == "ruler":
        assert rounds == 9 > ROUND_BATCH                                           # the driver goes through a second read-back


@pytest.mark.parametrize("numbering", ["random", "ruler"])
def test_scrambled_chain_round_caps(hip, numbering):
    """both callers keep their own failure path under their own cap: code 4, their outputs at -1"""
    import torch
    host, L = hip
    order = _scrambled_chains()[numbering]
    n = len(order)
    index, element, x, metals = _dev(_chain(order), np.int32), _dev(np.full(n, VACANCY), np.int32), _dev(np.zeros(n), np.float64), _dev([6], np.int32)
    host._use_stream(index.device)
    good = torch.zeros(n, dtype=torch.int32, device="cuda:0")                     # the labels of the finished labelling: one component, root 0
    label, role, bypass = (torch.full((n,), 7, dtype=torch.int32, device="cuda:0") for _ in range(3))
    L.dkmc_debug_set_cluster_round_cap(3)
    L.dkmc_debug_set_cut_round_cap(3)
    rc = L.dkmc_find_clusters(n, 2, host._ptr(index), host._ptr(element), None, host._ptr(x), host._ptr(metals), 1, cr.VACANCY_BIT, 1, 1, host._ptr(label))
    msg = L.dkmc_last_error().decode()
    L.dkmc_clear_error()
    assert rc == 4 and "dkmc_find_clusters" in msg and "3 rounds" in msg and (label.cpu().numpy() == -1).all()
    rc = L.dkmc_find_cuts(n, 2, host._ptr(index), host._ptr(good), None, 1, 1, None, 0, host._ptr(role), host._ptr(bypass))
    msg = L.dkmc_last_error().decode()
    L.dkmc_clear_error()
    assert rc == 4 and "dkmc_find_cuts" in msg and "3 rounds" in msg
    assert (role.cpu().numpy() == -1).all() and (bypass.cpu().numpy() == -1).all()
