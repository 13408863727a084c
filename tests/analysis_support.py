"""What the tests of the six filament analyses share (test_gpu_{clusters,gaps,paths,track,cuts,flow,shared_labelling}.py, the test_*_exports.py
and the test_*_ref.py of the analyses): the module-scoped `hip` fixture -- a test module imports it by name, so that it stays one instance per
module --, the host-to-device helper, the small graph builders, the shape list of the random-graph tests and the readers of the public headers.
No test of its own; no test module imports from another one."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# N, nn, p_member, p_pad of the random graphs: workgroup and wave edges, both row-lane templates (16 lanes up to nn = 128), the whole-wave row
SHAPES = [(1, 1, 1.0, 0.0), (7, 2, 0.8, 0.3), (40, 3, 0.5, 0.5), (63, 2, 0.9, 0.2), (150, 4, 0.3, 0.1),
          (255, 3, 0.7, 0.3), (256, 16, 0.5, 0.85), (257, 17, 0.6, 0.9), (1000, 1, 0.9, 0.1), (1000, 128, 0.5, 0.985), (1000, 130, 0.6, 0.99)]


@pytest.fixture(scope="module")
def hip():
    import torch
    import __graft_entry__ as g
    g.build()
    from devicekmc_amd import host, lib
    assert torch.cuda.is_available()
    return host, lib.load()


def _dev(a, dtype):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype).reshape(-1)).to("cuda:0")


# ---- graphs ---------------------------------------------------------------------------------------------------------------------------------
def _random_case(rng, N, nn, p_member, p_pad, one_way):
    """index with padding anywhere in a row; one_way: every link is entered in one of its two rows only"""
    index = rng.integers(0, N, size=(N, nn)).astype(np.int32)
    index[rng.random((N, nn)) < p_pad] = -1
    if one_way:
        rows = np.arange(N)[:, None]
        index[(index >= 0) & (index < rows)] = -1                       # row u keeps only v >= u
    element = np.where(rng.random(N) < p_member, rng.choice([2, 6], N), 3).astype(np.int32)
    charge = rng.integers(0, 2, N).astype(np.int32) * 2
    return index, element, charge, rng.normal(size=N) * 10.0


def _contacts(el, n):
    nondef = np.flatnonzero(el != 0)
    return int(nondef[n - 1]) + 1, len(el) - int(nondef[len(nondef) - n])


def _chain(order):
    """the sites of order linked in a row, both directions entered"""
    n = len(order)
    index = np.full((n, 2), -1, dtype=np.int32)
    index[order[:-1], 0] = order[1:]; index[order[1:], 1] = order[:-1]
    return index


def ordered_chain(n):
    """sites 0 ... n - 1 linked in a row, both directions entered: column 0 the site before, column 1 the one after"""
    return np.stack([np.arange(n) - 1, np.r_[np.arange(1, n), -1]], axis=1).astype(np.int32)


def ladder(length, first=0):
    """the links of two rails of `length` sites with a rung at every level: sites first + 2 i, first + 2 i + 1 are level i"""
    a = first + 2 * np.arange(length)
    return [(a[i], a[i + 1]) for i in range(length - 1)] + [(a[i] + 1, a[i + 1] + 1) for i in range(length - 1)] + [(a[i], a[i] + 1) for i in range(length)]


def index_of(links, n, nn=4):
    """each link entered once, in the row of its first end"""
    index = np.full((n, nn), -1, dtype=np.int32)
    fill = np.zeros(n, dtype=np.int64)
    for u, v in links:
        index[u, fill[u]] = v; fill[u] += 1
    return index


# ---- the public headers ---------------------------------------------------------------------------------------------------------------------
def _raw(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _code(name):
    return re.sub(r"/\*.*?\*/", " ", _raw(name), flags=re.S)


def _args(src, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]
