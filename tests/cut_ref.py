"""Host reference of the cut-site analysis (dkmc_find_cuts; definitions: include/devicekmc_hip.h): the members every conducting path between the
contacts crosses, by the rule of the off-path components and the chords of one left-to-right path, plus a brute force that deletes a member and
searches, a randomised simple path and the synchronous model of the off-path labelling's rounds (cluster_ref's; the link rows are path_ref's).
Everything it returns is an integer or one of the input doubles, so the device result is compared with np.array_equal."""
import numpy as np

import cluster_ref as cr
import path_ref as pr

INFO = ("status", "path_len", "cut_sites", "necks", "longest_neck", "longest_neck_first", "bypasses", "offpath_components", "offpath_members",
        "max_bypass", "chord_positions", "rounds")
PATH = ("site", "n_bypass", "chord", "cut")
BYPASSES = ("root", "size", "lo", "hi")
NECKS = ("first", "last", "xmin", "xmax")
NON_MEMBER, CUT, PATH_SITE, BYPASS, SIDE, APART = range(6)                  # the codes of site_role
NONE = 0x7fffffff


def graph(index, label, n_left, n_right):
    """-> (mask, ptr, nb, seeds_left, seeds_right): members, their links as rows in both directions, the clamped seeds"""
    label = np.asarray(label)
    N = len(label)
    n_left, n_right = min(max(int(n_left), 0), N), min(max(int(n_right), 0), N)
    mask = pr.member_mask(label, N)
    ids = np.arange(N)
    ptr, nb = pr.member_links(index, mask)
    return mask, ptr, nb, mask & (ids < n_left), mask & (ids >= N - n_right)


def model_rounds(ptr, nb, mask):
    """Rounds of the synchronous model the device runs (cluster_ref.hook_compress_rounds) on the members of mask, over the links between them
    only.  -> (rounds, root int64 [N]: the smallest site index of the component, -1 outside mask).  0 rounds at N == 0."""
    N = len(mask)
    if N == 0:
        return 0, np.zeros(0, dtype=np.int64)
    u = np.repeat(np.arange(N), np.diff(ptr))
    ok = mask[u] & mask[nb]
    return cr.hook_compress_rounds(u[ok], nb[ok], mask)


def check_path(path, N, mask, ptr, nb, seeds_left, seeds_right):
    """The device's validation: None, or (first offending row, reason)."""
    L = len(path)
    seen = {}
    for k in range(L):
        s = int(path[k])
        if s < 0 or s >= N or not mask[s]:
            return k, "not a member"
        if s in seen:
            return k, "a duplicate"
        seen[s] = k
        if k == 0 and not seeds_left[s]:
            return k, "row 0 is not a left seed"
        if k == L - 1 and not seeds_right[s]:
            return k, "the last row is not a right seed"
        if k > 0 and int(path[k - 1]) not in nb[ptr[s]:ptr[s + 1]]:
            return k, "not linked to the row before"
    return None


def analyse(index, label, x, n_left, n_right, path):
    """-> (site_role int32 [N], site_bypass int32 [N], path table dict of PATH (int32, len(path) rows), bypass table dict of BYPASSES (int32,
    ascending root), neck table dict of NECKS (first, last int32; xmin, xmax float64), info dict of INFO).  x may be None: the x columns then hold
    +inf / -inf.  An empty path is the status 0 answer; an invalid one raises ValueError naming the first offending row."""
    path = np.asarray(path, dtype=np.int64).reshape(-1)
    mask, ptr, nb, seeds_left, seeds_right = graph(index, label, n_left, n_right)
    N, L = len(mask), len(path)
    bad = check_path(path, N, mask, ptr, nb, seeds_left, seeds_right)
    if bad is not None:
        raise ValueError("path row %d: %s" % bad)
    pos = np.full(N, -1, dtype=np.int64)
    pos[path] = np.arange(L)
    off = mask & (pos < 0)
    rounds, root = model_rounds(ptr, nb, off)
    bypass = root.astype(np.int32)
    # attachments of the off-path components: the path positions linked to them, -1 with a left seed, L with a right seed
    lo, hi = np.full(N, NONE, dtype=np.int64), np.full(N, -NONE, dtype=np.int64)
    bdiff, cdiff = np.zeros(L + 1, dtype=np.int64), np.zeros(L + 1, dtype=np.int64)
    if L:
        u = np.repeat(np.arange(N), np.diff(ptr))
        a = off[u] & (pos[nb] >= 0)
        np.minimum.at(lo, root[u[a]], pos[nb[a]]); np.maximum.at(hi, root[u[a]], pos[nb[a]])
        s = np.flatnonzero(off & seeds_left)
        np.minimum.at(lo, root[s], -1); np.maximum.at(hi, root[s], -1)
        s = np.flatnonzero(off & seeds_right)
        np.minimum.at(lo, root[s], L); np.maximum.at(hi, root[s], L)
        # chords: links between two path sites two or more positions apart, path sites that are seeds away from their end
        c = (pos[u] >= 0) & (pos[nb] >= pos[u] + 2)
        np.add.at(cdiff, pos[u[c]] + 1, 1); np.add.at(cdiff, pos[nb[c]], -1)
        k = np.flatnonzero(seeds_left[path] & (np.arange(L) >= 1))
        cdiff[0] += len(k); np.add.at(cdiff, k, -1)
        k = np.flatnonzero(seeds_right[path] & (np.arange(L) <= L - 2))
        np.add.at(cdiff, k + 1, 1); cdiff[L] -= len(k)
    roots = np.flatnonzero(off & (root == np.arange(N)))
    attached = lo[roots] != NONE
    wide = attached & (hi[roots] - lo[roots] >= 2)
    broots = roots[wide]
    np.add.at(bdiff, lo[broots] + 1, 1); np.add.at(bdiff, hi[broots], -1)
    n_bypass = np.cumsum(bdiff)[:L].astype(np.int32)
    chord = (np.cumsum(cdiff)[:L] > 0).astype(np.int32)
    cut = ((n_bypass == 0) & (chord == 0)).astype(np.int32)
    table = dict(site=path.astype(np.int32), n_bypass=n_bypass, chord=chord, cut=cut)
    size = np.bincount(root[off], minlength=N) if N else np.zeros(0, dtype=np.int64)
    bypasses = dict(root=broots.astype(np.int32), size=size[broots].astype(np.int32), lo=lo[broots].astype(np.int32), hi=hi[broots].astype(np.int32))
    # roles
    role = np.zeros(N, dtype=np.int32)
    kind = np.full(N, APART, dtype=np.int32)
    kind[roots[attached]] = SIDE
    kind[broots] = BYPASS
    role[off] = kind[root[off]]
    role[path] = np.where(cut == 1, CUT, PATH_SITE)
    # necks: the maximal runs of consecutive cut positions
    padded = np.r_[0, cut, 0]
    first, last = np.flatnonzero(np.diff(padded) == 1), np.flatnonzero(np.diff(padded) == -1) - 1
    xmin, xmax = np.full(len(first), np.inf), np.full(len(first), -np.inf)
    if x is not None:
        x = np.asarray(x, dtype=np.float64)
        for j, (a, b) in enumerate(zip(first, last)):
            xmin[j], xmax[j] = x[path[a:b + 1]].min(), x[path[a:b + 1]].max()
    necks = dict(first=first.astype(np.int32), last=last.astype(np.int32), xmin=xmin, xmax=xmax)
    length = last - first + 1
    j = int(np.argmax(length)) if len(first) else -1                       # the first of the longest
    info = dict(status=int(L > 0), path_len=L, cut_sites=int(cut.sum()), necks=len(first), longest_neck=int(length[j]) if j >= 0 else 0,
                longest_neck_first=int(first[j]) if j >= 0 else -1, bypasses=len(broots), offpath_components=len(roots),
                offpath_members=int(off.sum()), max_bypass=int(n_bypass.max()) if L else 0, chord_positions=int(chord.sum()), rounds=int(rounds))
    return role, bypass, table, bypasses, necks, info


def brute_cut_set(index, label, n_left, n_right, sites=None):
    """The definition itself: the members v (of sites, by default all members), ascending, after whose deletion no left seed other than v is
    connected to a right seed other than v."""
    mask, ptr, nb, seeds_left, seeds_right = graph(index, label, n_left, n_right)
    sites = np.flatnonzero(mask) if sites is None else np.unique(np.asarray(sites, dtype=np.int64))
    out = []
    for v in sites:
        assert mask[v]
        seen = seeds_left.copy()
        seen[v] = False
        front = np.flatnonzero(seen)
        while len(front):
            t = np.unique(pr.linked(ptr, nb, front))
            t = t[~seen[t] & (t != v)]
            seen[t] = True
            front = t
        if not (seen & seeds_right).any():
            out.append(int(v))
    return np.array(out, dtype=np.int32)


def random_simple_path(rng, ptr, nb, seeds_left, seeds_right, p_stop=0.6):
    """A randomised depth-first walk from a random left seed; it ends at the first right seed it keeps (one it reaches is kept with probability
    p_stop, and always when the walk cannot go on from it).  -> int32 sites of a simple path, empty if the walk finds no right seed."""
    starts = [int(s) for s in rng.permutation(np.flatnonzero(seeds_left))]
    visited = np.zeros(len(seeds_left), dtype=bool)
    stack = []
    while stack or starts:
        if not stack:                                                       # the next left seed no earlier walk came through
            s = starts.pop()
            if not visited[s]:
                visited[s] = True
                stack.append(s)
            continue
        a = stack[-1]
        nxt = np.unique(nb[ptr[a]:ptr[a + 1]])
        nxt = nxt[~visited[nxt]]
        if seeds_right[a] and (len(nxt) == 0 or rng.random() < p_stop):
            return np.array(stack, dtype=np.int32)
        if len(nxt) == 0:
            stack.pop()                                                     # a dead end: the site stays visited, the walk backs up
            continue
        b = int(rng.choice(nxt))
        visited[b] = True
        stack.append(b)
    return np.zeros(0, dtype=np.int32)


def assert_equal(role, bypass, table, bypasses, necks, info, ref, rows=None):
    """Device result against analyse(): array_equal everywhere, doubles included."""
    r_role, r_bypass, r_table, r_byp, r_necks, r_info = ref
    assert np.asarray(role).dtype == np.int32 and np.array_equal(np.asarray(role), r_role)
    assert np.asarray(bypass).dtype == np.int32 and np.array_equal(np.asarray(bypass), r_bypass)
    for names, got, want in ((PATH, table, r_table), (BYPASSES, bypasses, r_byp), (NECKS, necks, r_necks)):
        for k in names:
            n = len(want[k]) if rows is None else min(rows, len(want[k]))
            assert got[k].dtype == want[k].dtype, k
            assert np.array_equal(got[k], want[k][:n]), k
    for k in INFO:
        assert info[k] == r_info[k], (k, info[k], r_info[k])


# ---- pinned cases (tests/test_cut_ref.py, tests/test_gpu_cuts.py, tests/test_flow_ref.py) --------------------------------------------------
# the figures of the planted filaments of the 2.5 nm golden device: the reference and the device are pinned to the same ones.  radius: path_len, the cut positions, necks,
# longest neck, its first position, bypass components
PINNED_2P5 = {3.0: (48, [], 0, 0, -1, 1), 2.6: (48, [12], 1, 1, 12, 3), 2.4: (48, [12, 13, 14], 1, 3, 12, 4),
              2.2: (48, [12, 13, 14, 19, 25, 26, 31], 4, 3, 12, 8)}
PINNED_2P5_WIDE_BYPASS = (0, 3483, -1, 48)                                  # r = 3.0: the one bypass component's root, size, lo, hi


def planted_2p5(s, p, el, neigh, r):
    from analysis_support import _contacts
    el2, _ = cr.plant_filament(el, s.x, s.y, s.z, r)
    nl, nr = _contacts(el2, p.num_atoms_first_layer)
    label = np.where(cr.member_mask(el2, None, list(p.metals), cr.METAL | cr.VACANCY_BIT), 0, -1).astype(np.int32)
    path = pr.analyse(neigh, label, s.x, nl, nr, 0)[2]
    return label, nl, nr, path
