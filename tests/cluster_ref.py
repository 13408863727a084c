"""Host reference of the filament analysis (dkmc_find_clusters; definitions: include/devicekmc_hip.h): labels, component table and info from
scipy's connected components, relabelled to the smallest site index, plus the synchronous model of the labelling's rounds.  Everything it returns
is an integer or one of the input doubles, so the device result is compared with np.array_equal."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

METAL, VACANCY_BIT, NEUTRAL_ONLY = 1, 2, 4
VACANCY_EL = 2                                   # ELEMENT::VACANCY (utils.h:37-44)
INFO_INT = ("n_members", "n_components", "bridged", "bridge_root", "largest_free_size", "rounds")
TABLE = ("root", "size", "n_vacancy", "flags", "xmin", "xmax")


def member_mask(element, charge, metals, members):
    element = np.asarray(element)
    m = np.zeros(len(element), dtype=bool)
    if members & METAL:
        m |= np.isin(element, np.asarray(metals))
    if members & VACANCY_BIT:
        v = element == VACANCY_EL
        if members & NEUTRAL_ONLY:
            v &= np.asarray(charge) == 0
        m |= v
    return m


def member_edges(index, mask):
    """(u, v) of every index entry between two members; entries < 0 or >= N are padding."""
    N = len(mask)
    index = np.asarray(index).reshape(N, -1) if N else np.zeros((0, 1), dtype=np.int32)
    u = np.repeat(np.arange(N), index.shape[1])
    v = index.reshape(-1).astype(np.int64)
    ok = (v >= 0) & (v < N)
    u, v = u[ok], v[ok]
    ok = mask[u] & mask[v]
    return u[ok], v[ok]


def labels_of(index, mask):
    N = len(mask)
    u, v = member_edges(index, mask)
    g = sp.coo_matrix((np.ones(len(u), dtype=np.int8), (u, v)), shape=(N, N)).tocsr()
    _, comp = connected_components(g, directed=False)                       # one-directional entries link too
    ids = np.flatnonzero(mask)
    smallest = np.full(comp.max() + 1 if N else 0, N, dtype=np.int64)
    np.minimum.at(smallest, comp[ids], ids)
    label = np.full(N, -1, dtype=np.int32)
    label[ids] = smallest[comp[ids]]
    return label


def hook_compress_rounds(u, v, mask):
    """The synchronous model of the device's labelling on the links (u[k], v[k]) between members of mask: every round hooks, for every link whose
    ends have different roots, the larger root under the smaller (minimum per root), then compresses every member to its root; the round in which
    nothing is hooked counts.  -> (rounds, root int64 [N]: the smallest site index of the component, -1 outside mask)."""
    N = len(mask)
    root = np.where(mask, np.arange(N), -1).astype(np.int64)
    rounds = 0
    while True:
        rounds += 1
        ru, rv = root[u], root[v]
        d = ru != rv
        if not d.any():
            return rounds, root
        parent = np.arange(N)
        np.minimum.at(parent, np.maximum(ru[d], rv[d]), np.minimum(ru[d], rv[d]))
        while True:                                                         # pointer doubling to the roots
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
        root = np.where(mask, parent[np.where(mask, root, 0)], -1)


def model_rounds(index, mask):
    """Rounds (and final roots) of hook_compress_rounds over every index entry between two members."""
    return hook_compress_rounds(*member_edges(index, mask), mask)


def analyse(index, element, charge, x, metals, members, n_left, n_right, with_rounds=True):
    """-> (label int32 [N], table dict of arrays (all rows, ascending root), info dict)."""
    element = np.asarray(element); x = np.asarray(x, dtype=np.float64)
    N = len(element)
    n_left, n_right = min(max(int(n_left), 0), N), min(max(int(n_right), 0), N)
    mask = member_mask(element, charge, metals, members)
    label = labels_of(index, mask)
    ids = np.flatnonzero(mask)
    roots, inv = np.unique(label[ids], return_inverse=True)
    nc = len(roots)
    size = np.bincount(inv, minlength=nc).astype(np.int32)
    nvac = np.bincount(inv, weights=(element[ids] == VACANCY_EL), minlength=nc).astype(np.int32)
    flags = np.zeros(nc, dtype=np.int32)
    np.bitwise_or.at(flags, inv, ((ids < n_left) * 1 + (ids >= N - n_right) * 2).astype(np.int32))
    xmin = np.full(nc, np.inf); xmax = np.full(nc, -np.inf)
    np.minimum.at(xmin, inv, x[ids]); np.maximum.at(xmax, inv, x[ids])
    table = dict(root=roots.astype(np.int32), size=size, n_vacancy=nvac, flags=flags, xmin=xmin, xmax=xmax)
    both = flags == 3
    bridged = int(both.any())
    left, right, free = flags == 1, flags == 2, flags == 0
    tl = float(xmax[left].max()) if left.any() else -np.inf
    tr = float(xmin[right].min()) if right.any() else np.inf
    info = dict(n_members=int(len(ids)), n_components=int(nc), bridged=bridged, bridge_root=int(roots[both].min()) if bridged else -1,
                largest_free_size=int(size[free].max()) if free.any() else 0,
                tip_left_x=tl, tip_right_x=tr, gap_x=0.0 if bridged else tr - tl)
    if with_rounds:
        info["rounds"], root = model_rounds(index, mask)
        assert np.array_equal(root.astype(np.int32), label)                # the model ends on the canonical labels
    return label, table, info


def flood_fill(index, mask):
    """Brute force for small graphs: symmetric adjacency sets, depth-first fill in ascending order of the seed."""
    N = len(mask)
    index = np.asarray(index).reshape(N, -1)
    adj = [set() for _ in range(N)]
    for a in range(N):
        for b in index[a]:
            if 0 <= b < N and mask[a] and mask[b]:
                adj[a].add(int(b)); adj[int(b)].add(a)
    label = np.full(N, -1, dtype=np.int32)
    for s in range(N):
        if mask[s] and label[s] < 0:
            stack = [s]; label[s] = s
            while stack:
                a = stack.pop()
                for b in adj[a]:
                    if label[b] < 0:
                        label[b] = s; stack.append(b)
    return label


def plant_filament(element, x, y, z, r, skip=None, o_el=3):
    """The planted filament of the tests: every O site within r of the device's axis (medians over all sites) becomes a VACANCY, optionally
    leaving out skip[0] < x < skip[1].  Returns (new element array, sites planted)."""
    d = np.hypot(y - np.median(y), z - np.median(z))
    sel = (np.asarray(element) == o_el) & (d < r)
    if skip is not None:
        sel &= ~((x > skip[0]) & (x < skip[1]))
    el = np.array(element, dtype=np.int32, copy=True)
    el[sel] = VACANCY_EL
    return el, int(sel.sum())


def assert_equal(label, table, info, ref, rows=None):
    """Device result against analyse(): array_equal everywhere, doubles included."""
    rl, rt, ri = ref
    assert np.array_equal(np.asarray(label), rl)
    n = len(rt["root"]) if rows is None else rows
    for k in TABLE:
        assert table[k].dtype == rt[k].dtype, k
        assert np.array_equal(table[k], rt[k][:n]), k
    for k in ri:
        assert info[k] == ri[k], (k, info[k], ri[k])
