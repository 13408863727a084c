"""Host reference of the gap analysis (dkmc_find_gaps; definitions: include/devicekmc_hip.h), numpy only: brute force over all member pairs with
the contract's arithmetic (every product and every sum rounded on its own), Kruskal under the strict key order (d2, a, b) with the contact nodes
merged beforehand, the L -> R tree path, the direct gap, and the synchronous model of the Boruvka rounds.  Every number it returns is an integer
or a d2 of that arithmetic, so the device result is compared with np.array_equal.  Meant for a few thousand members."""
import numpy as np

EDGES = ("site_a", "site_b", "root_a", "root_b", "d2", "dist")
CHAIN = ("from_site", "to_site", "d2", "dist")
INFO_PINNED = ("n_components", "n_edges", "status", "n_hops", "rounds", "direct", "bottleneck_d2", "bottleneck")


def c_round(f):
    """round() of C: halves away from zero (np.round goes to even)"""
    t = np.trunc(f)
    return np.where(np.abs(f - t) >= 0.5, t + np.copysign(1.0, f), t)


def pair_d2(a, b, x, y, z, lattice, pbc):
    """d2 of the site pairs (a, b), a < b elementwise"""
    dx = x[a] - x[b]
    dy = y[a] - y[b]
    dz = z[a] - z[b]
    if pbc:
        fy = dy / lattice[1]
        fy = fy - c_round(fy)
        fz = dz / lattice[2]
        fz = fz - c_round(fz)
        dy = fy * lattice[1]
        dz = fz * lattice[2]
    return (dx * dx + dy * dy) + dz * dz


def nodes_of(label, n_left, n_right):
    """-> (ids of the members, node per member, n_components, has_left, has_right, bridged).  Node N is L, N + 1 is R (N too when bridged)."""
    label = np.asarray(label)
    N = len(label)
    n_left, n_right = min(max(int(n_left), 0), N), min(max(int(n_right), 0), N)
    ids = np.flatnonzero((label >= 0) & (label < N))
    lab = label[ids].astype(np.int64)
    flags = np.zeros(N + 1, dtype=np.int64)
    np.bitwise_or.at(flags, lab, (ids < n_left) * 1 + (ids >= N - n_right) * 2)
    f = flags[lab]
    bridged = bool((f == 3).any())
    node = np.where(f == 0, lab, np.where(((f & 1) != 0) | bridged, N, N + 1))
    return ids, node, len(np.unique(lab)), bool((f & 1).any()), bool((f & 2).any()), bridged


def candidates(label, x, y, z, lattice, pbc, n_left, n_right, r_max):
    """All candidate edges, sorted by the key: (a, b, d2, node_a, node_b) + what nodes_of returns"""
    x, y, z = (np.asarray(v, dtype=np.float64) for v in (x, y, z))
    ids, node, ncomp, has_l, has_r, bridged = nodes_of(label, n_left, n_right)
    iu, iv = np.triu_indices(len(ids), 1)
    keep = node[iu] != node[iv]
    iu, iv = iu[keep], iv[keep]
    a, b = ids[iu], ids[iv]                                                  # ids ascend: a < b
    d2 = pair_d2(a, b, x, y, z, lattice, pbc)
    keep = d2 <= np.float64(r_max) * np.float64(r_max)
    a, b, d2, na, nb = a[keep], b[keep], d2[keep], node[iu[keep]], node[iv[keep]]
    o = np.lexsort((b, a, d2))
    return (a[o], b[o], d2[o], na[o], nb[o]), (ncomp, has_l, has_r, bridged)


class _Sets:
    def __init__(self):
        self.p = {}

    def find(self, v):
        p = self.p
        r = v
        while p.setdefault(r, r) != r:
            r = p[r]
        while p[v] != r:
            p[v], v = r, p[v]
        return r

    def union(self, u, v):
        ru, rv = self.find(u), self.find(v)
        if ru == rv:
            return False
        self.p[max(ru, rv)] = min(ru, rv)
        return True


def _lightest_per_node_pair(na, nb):
    """positions (ascending, i.e. in key order) of the first edge of every unordered node pair: the only ones a spanning forest can use"""
    lo, hi = np.minimum(na, nb), np.maximum(na, nb)
    _, first = np.unique(lo * (hi.max() + 1 if len(hi) else 1) + hi, return_index=True)
    return np.sort(first)


def kruskal(na, nb):
    """positions of the forest's edges among the key-sorted candidates"""
    s, out = _Sets(), []
    for k in _lightest_per_node_pair(na, nb):
        if s.union(int(na[k]), int(nb[k])):
            out.append(int(k))
    return out


def boruvka(na, nb):
    """The synchronous rounds: every node picks its lightest candidate edge to another node, all picks are contracted, until a round in which no
    node has a candidate; that round counts.  -> (rounds, positions of the picked edges, ascending)"""
    pos = _lightest_per_node_pair(na, nb)
    s, picked, rounds = _Sets(), set(), 0
    while True:
        rounds += 1
        best = {}
        for k in pos:                                                           # key order: the first edge seen by a node is its lightest
            u, v = s.find(int(na[k])), s.find(int(nb[k]))
            if u != v:
                best.setdefault(u, int(k)); best.setdefault(v, int(k))
        if not best:
            return rounds, sorted(picked)
        for k in set(best.values()):
            s.union(int(na[k]), int(nb[k]))
            picked.add(k)


def tree_path(na, nb, forest, src, dst):
    """positions of the forest edges on the path src -> dst, in order, with the node each hop leaves from; None when they lie in different trees"""
    adj = {}
    for k in forest:
        adj.setdefault(int(na[k]), []).append((k, int(nb[k])))
        adj.setdefault(int(nb[k]), []).append((k, int(na[k])))
    via, todo = {src: None}, [src]
    while todo:
        v = todo.pop()
        for k, w in adj.get(v, []):
            if w not in via:
                via[w] = (k, v); todo.append(w)
    if dst not in via:
        return None
    path, v = [], dst
    while via[v] is not None:
        k, u = via[v]
        path.append((k, u)); v = u
    return path[::-1]


def analyse(label, x, y, z, lattice, pbc, n_left, n_right, r_max):
    """-> (edges, chain, info): dicts as devicekmc_amd.host.find_gaps returns them (info without pairs_tested)"""
    label = np.asarray(label)
    N = len(label)
    (a, b, d2, na, nb), (ncomp, has_l, has_r, bridged) = candidates(label, x, y, z, lattice, pbc, n_left, n_right, r_max)
    forest = kruskal(na, nb)
    rounds, picked = boruvka(na, nb)
    assert picked == forest                                                     # the forest is unique under a strict order
    f = np.asarray(forest, dtype=np.int64)
    edges = dict(site_a=a[f].astype(np.int32), site_b=b[f].astype(np.int32), root_a=label[a[f]].astype(np.int32), root_b=label[b[f]].astype(np.int32),
                 d2=d2[f], dist=np.sqrt(d2[f]))
    status, hops, direct, bott = 0, [], None, np.inf
    if bridged:
        status, bott = 2, 0.0
    elif has_l and has_r:
        path = tree_path(na, nb, forest, N, N + 1)
        if path is not None:
            status = 1
            hops = [((a[k], b[k]) if na[k] == u else (b[k], a[k])) + (d2[k],) for k, u in path]
            bott = max(h[2] for h in hops)
        lr = np.flatnonzero(np.minimum(na, nb) == N)
        lr = lr[np.maximum(na, nb)[lr] == N + 1]
        if len(lr):
            k = lr[0]
            direct = (int(a[k]), int(b[k]), float(np.sqrt(d2[k])))
    cd2 = np.array([h[2] for h in hops], dtype=np.float64)
    chain = dict(from_site=np.array([h[0] for h in hops], dtype=np.int32), to_site=np.array([h[1] for h in hops], dtype=np.int32), d2=cd2,
                 dist=np.sqrt(cd2))
    info = dict(n_components=ncomp, n_edges=len(forest), status=status, n_hops=len(hops), rounds=rounds, direct=direct,
                bottleneck_d2=float(bott), bottleneck=float(np.sqrt(bott)))
    return edges, chain, info


def assert_equal(edges, chain, info, ref, rows=None, chain_rows=None):
    """Device result against analyse(): array_equal on every integer and every d2 (and on the square roots numpy takes of them)"""
    re_, rc, ri = ref
    n = len(re_["d2"]) if rows is None else rows
    for k in EDGES:
        assert edges[k].dtype == re_[k].dtype, k
        assert np.array_equal(edges[k], re_[k][:n]), k
    n = len(rc["d2"]) if chain_rows is None else chain_rows
    for k in CHAIN:
        assert chain[k].dtype == rc[k].dtype, k
        assert np.array_equal(chain[k], rc[k][:n]), k
    for k in INFO_PINNED:
        assert info[k] == ri[k], (k, info[k], ri[k])
