"""The host reference of the conduction-path analysis (path_ref.py) checked on its own: against a brute force (adjacency sets, a deque
breadth-first search per seed set, exhaustive predecessor minimisation) on small random graphs, and on the planted filaments of the two golden
devices, whose figures are pinned here.  No GPU."""
from collections import deque

import numpy as np
import pytest

import cluster_ref as cr
import path_ref as pr
from conftest import params_7p5
from path_ref import PINNED_2P5_BRIDGED, PINNED_7P5_BRIDGED
from analysis_support import _contacts, _random_case


def _brute(index, label, x, n_left, n_right, slack):
    N = len(label)
    index = np.asarray(index).reshape(N, -1)
    mem = [0 <= int(label[i]) < N for i in range(N)]
    adj = [set() for _ in range(N)]
    for a in range(N):
        for b in index[a]:
            if 0 <= b < N and mem[a] and mem[int(b)]:
                adj[a].add(int(b)); adj[int(b)].add(a)
    n_left, n_right = min(max(n_left, 0), N), min(max(n_right, 0), N)

    def bfs(seeds):
        hop = [-1] * N
        q = deque()
        for s in seeds:
            hop[s] = 0; q.append(s)
        while q:
            a = q.popleft()
            for b in adj[a]:
                if hop[b] < 0:
                    hop[b] = hop[a] + 1; q.append(b)
        return hop

    left = [i for i in range(N) if mem[i] and i < n_left]
    right = [i for i in range(N) if mem[i] and i >= N - n_right]
    hl, hr = bfs(left), bfs(right)
    ends = [i for i in right if hl[i] >= 0]
    largest = max(hl + hr + [0])
    out = dict(hl=hl, hr=hr, rounds=(largest + 1) if N else 0, status=int(bool(ends)))
    if ends:
        H = min(hl[i] for i in ends)
        path = [min(i for i in ends if hl[i] == H)]
        for k in range(H, 0, -1):
            path.append(min(b for b in adj[path[-1]] if hl[b] == k - 1))
        cor = [i for i in range(N) if hl[i] >= 0 and hr[i] >= 0 and hl[i] + hr[i] <= H + slack]
        rows = [[i for i in cor if hl[i] == k] for k in range(H + slack + 1)]
        out.update(H=H, path=path[::-1], cor=cor, rows=rows)
    return out


def _check(index, label, x, nl, nr, slack):
    N = len(label)
    hl, hr, path, prof, info = pr.analyse(index, label, x, nl, nr, slack)
    b = _brute(index, label, x, nl, nr, slack)
    assert hl.dtype == np.int32 and hr.dtype == np.int32 and hl.tolist() == b["hl"] and hr.tolist() == b["hr"]
    assert info["rounds"] == b["rounds"] and info["status"] == b["status"]
    assert info["reached_left"] == sum(h >= 0 for h in b["hl"]) and info["reached_right"] == sum(h >= 0 for h in b["hr"])
    if not b["status"]:
        assert (info["hops"], info["corridor_sites"], info["constriction_level"], info["constriction_width"]) == (-1, 0, -1, 0)
        assert len(path) == 0 and all(len(prof[k]) == 0 for k in pr.PROFILE)
        return info
    H = b["H"]
    assert info["hops"] == H == min(b["hr"][i] for i in range(min(max(nl, 0), N)) if b["hr"][i] >= 0)
    assert path.tolist() == b["path"] and info["corridor_sites"] == len(b["cor"])
    assert prof["count"].tolist() == [len(r) for r in b["rows"]]
    for k, r in enumerate(b["rows"]):
        assert prof["xmin"][k] == (min(x[i] for i in r) if r else np.inf) and prof["xmax"][k] == (max(x[i] for i in r) if r else -np.inf)
    widths = [len(r) for r in b["rows"][:H + 1]]
    assert min(widths) >= 1
    assert (info["constriction_level"], info["constriction_width"]) == (widths.index(min(widths)), min(widths))
    return info


@pytest.mark.parametrize("one_way", [False, True])
@pytest.mark.parametrize("N,nn,p_member,p_pad", [(1, 1, 1.0, 0.0), (7, 2, 0.8, 0.3), (40, 3, 0.5, 0.5), (63, 2, 0.9, 0.2), (150, 4, 0.3, 0.1)])
def test_reference_equals_brute_force(N, nn, p_member, p_pad, one_way):
    rng = np.random.default_rng(1000 * N + nn + one_way)
    connected = 0
    for trial in range(6):
        index, element, _, x = _random_case(rng, N, nn, p_member, p_pad, one_way)
        label = np.where(element != 3, rng.integers(0, N, N), rng.choice([-1, N, N + 7, -5], N)).astype(np.int32)
        for nl, nr in ((N // 4, N // 4), (0, N // 3), (N // 3, 0), (0, 0), (N, N), (-3, 2 * N)):
            for slack in (0, 1, 3):
                connected += _check(index, label, x, nl, nr, slack)["status"]
    assert connected > 0


def test_empty_and_memberless_inputs():
    hl, hr, path, prof, info = pr.analyse(np.zeros((0, 3), dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0), 0, 0, 2)
    assert len(hl) == len(hr) == len(path) == len(prof["count"]) == 0 and info["status"] == 0 and info["rounds"] == 0 and info["hops"] == -1
    hl, hr, _, _, info = pr.analyse(np.array([[1], [0]], dtype=np.int32), np.array([-1, 2], dtype=np.int32), None, 1, 1, 0)
    assert hl.tolist() == [-1, -1] and hr.tolist() == [-1, -1] and info["status"] == 0 and info["rounds"] == 1


def test_chain_and_missing_x():
    """an ordered chain of n sites: H = n - 1, rounds = n, every level one site wide; without x the profile's x columns stay at +inf / -inf"""
    n = 30
    chain = np.stack([np.arange(n) - 1, np.r_[np.arange(1, n), -1]], axis=1).astype(np.int32)
    hl, hr, path, prof, info = pr.analyse(chain, np.zeros(n, dtype=np.int32), None, 1, 1, 2)
    assert hl.tolist() == list(range(n)) and hr.tolist() == list(range(n))[::-1] and path.tolist() == list(range(n))
    assert (info["hops"], info["rounds"], info["corridor_sites"], info["constriction_level"], info["constriction_width"]) == (n - 1, n, n, 0, 1)
    assert prof["count"].tolist() == [1] * n + [0, 0] and np.isposinf(prof["xmin"]).all() and np.isneginf(prof["xmax"]).all()


@pytest.fixture(scope="module")
def device_2p5(cell_2p5):
    from devicekmc_amd import params, structure
    p = params.KMCParameters()
    el, neigh, nn, _ = structure.prepare_device(cell_2p5, p, None)
    return cell_2p5, p, el, neigh, nn


def _planted(s, p, el, neigh, r, skip, slack):
    el2, _ = cr.plant_filament(el, s.x, s.y, s.z, r, skip)
    nl, nr = _contacts(el2, p.num_atoms_first_layer)
    label = np.where(cr.member_mask(el2, None, list(p.metals), cr.METAL | cr.VACANCY_BIT), 0, -1).astype(np.int32)
    return pr.analyse(neigh, label, s.x, nl, nr, slack)


@pytest.mark.parametrize("slack", [0, 2, 4])
def test_pinned_bridged_filament_2p5(device_2p5, slack):
    s, p, el, neigh, nn = device_2p5
    hl, hr, path, prof, info = _planted(s, p, el, neigh, 3.0, None, slack)
    assert (info["status"], info["hops"], info["rounds"], info["reached_left"], info["reached_right"]) == (1, 47, 49, 3533, 3533)
    assert (info["corridor_sites"], info["constriction_level"], info["constriction_width"]) == PINNED_2P5_BRIDGED[slack]
    assert len(path) == 48 and len(prof["count"]) == 48 + slack and int(prof["count"].sum()) == info["corridor_sites"]
    assert (prof["count"][:48] >= 1).all() and np.array_equal(hl[path], np.arange(48))


@pytest.mark.parametrize("r,skip,reached,largest", [(3.0, (25.0, 40.0), (1500, 2004), (21, 21)), (2.0, None, (1454, 2022), None)])
def test_pinned_open_filaments_2p5(device_2p5, r, skip, reached, largest):
    s, p, el, neigh, nn = device_2p5
    hl, hr, path, prof, info = _planted(s, p, el, neigh, r, skip, 2)
    assert info["status"] == 0 and info["hops"] == -1 and len(path) == 0 and len(prof["count"]) == 0
    assert (info["reached_left"], info["reached_right"]) == reached
    assert info["rounds"] == max(hl.max(), hr.max()) + 1
    if largest:
        assert (int(hl.max()), int(hr.max())) == largest


@pytest.mark.parametrize("slack", [0, 2])
def test_pinned_bridged_filament_7p5(dev_7p5, slack):
    from devicekmc_amd import structure
    p = params_7p5()
    el, neigh, nn, _ = structure.prepare_device(dev_7p5, p, None)
    hl, hr, path, prof, info = _planted(dev_7p5, p, el, neigh, 3.0, None, slack)
    assert (info["status"], info["hops"], info["rounds"], info["reached_left"], info["reached_right"]) == (1, 45, 59, 30963, 30963)
    assert (info["corridor_sites"], info["constriction_level"], info["constriction_width"]) == PINNED_7P5_BRIDGED[slack]
    if slack == 2:
        assert prof["count"][46:].tolist() == [233, 125]
