"""Host reference of the conduction-path analysis (dkmc_find_paths; definitions: include/devicekmc_hip.h): hop distances from both contacts over the
member links, the canonical shortest path, the corridor's level profile, its constriction and the synchronous model of the labelling's rounds.
numpy only.  Everything it returns is an integer or one of the input doubles, so the device result is compared with np.array_equal."""
import numpy as np

INFO = ("status", "hops", "rounds", "reached_left", "reached_right", "corridor_sites", "constriction_level", "constriction_width")
PROFILE = ("count", "xmin", "xmax")


def member_mask(label, N):
    label = np.asarray(label)
    return (label >= 0) & (label < N)


def member_links(index, mask):
    """The links between members in both directions, as rows: (ptr int64 [N + 1], nb int64 [ptr[N]]), the members linked to site i are
    nb[ptr[i]:ptr[i + 1]] (with repeats).  Entries < 0 or >= N are padding, anywhere in a row."""
    N = len(mask)
    index = np.asarray(index).reshape(N, -1) if N else np.zeros((0, 1), dtype=np.int32)
    u = np.repeat(np.arange(N), index.shape[1])
    v = index.reshape(-1).astype(np.int64)
    ok = (v >= 0) & (v < N)
    u, v = u[ok], v[ok]
    ok = mask[u] & mask[v]
    u, v = np.concatenate([u[ok], v[ok]]), np.concatenate([v[ok], u[ok]])
    order = np.argsort(u, kind="stable")
    return np.searchsorted(u[order], np.arange(N + 1)), v[order]


def linked(ptr, nb, sites):
    """every member linked to one of sites (with repeats)"""
    sites = np.asarray(sites, dtype=np.int64)
    cnt = ptr[sites + 1] - ptr[sites]
    total = int(cnt.sum())
    if total == 0:
        return np.zeros(0, dtype=np.int64)
    first = np.repeat(ptr[sites] - (np.cumsum(cnt) - cnt), cnt)
    return nb[first + np.arange(total)]


def model_rounds(ptr, nb, seeds_left, seeds_right):
    """The synchronous rounds the device runs: round k sets hop k + 1 in both fields from the sites that hold k; the first round that sets nothing
    in either field ends the loop and is counted.  -> (hops_left, hops_right, rounds)"""
    N = len(seeds_left)
    hl = np.where(seeds_left, 0, -1).astype(np.int32)
    hr = np.where(seeds_right, 0, -1).astype(np.int32)
    if N == 0:
        return hl, hr, 0
    k = 0
    while True:
        changed = False
        for h in (hl, hr):
            t = linked(ptr, nb, np.flatnonzero(h == k))
            t = t[h[t] == -1]
            if len(t):
                h[t] = k + 1
                changed = True
        k += 1
        if not changed:
            return hl, hr, k


def search(index, label, n_left, n_right):
    """The part of analyse() that does not depend on x and slack; analyse(searched=...) takes it, so that one search serves several slacks."""
    label = np.asarray(label)
    N = len(label)
    n_left, n_right = min(max(int(n_left), 0), N), min(max(int(n_right), 0), N)
    mask = member_mask(label, N)
    ids = np.arange(N)
    seeds_left, seeds_right = mask & (ids < n_left), mask & (ids >= N - n_right)
    ptr, nb = member_links(index, mask)
    hl, hr, rounds = model_rounds(ptr, nb, seeds_left, seeds_right)
    return ptr, nb, seeds_left, seeds_right, hl, hr, rounds


def analyse(index, label, x, n_left, n_right, slack, searched=None):
    """-> (hops_left int32 [N], hops_right int32 [N], path int32 [H + 1] (empty at status 0), profile dict of count int32 / xmin / xmax
    [H + slack + 1] (empty at status 0), info dict of INFO).  x may be None: the x columns then hold +inf / -inf."""
    ptr, nb, seeds_left, seeds_right, hl, hr, rounds = search(index, label, n_left, n_right) if searched is None else searched
    info = dict(status=0, hops=-1, rounds=int(rounds), reached_left=int((hl >= 0).sum()), reached_right=int((hr >= 0).sum()),
                corridor_sites=0, constriction_level=-1, constriction_width=0)
    path = np.zeros(0, dtype=np.int32)
    profile = dict(count=np.zeros(0, dtype=np.int32), xmin=np.zeros(0), xmax=np.zeros(0))
    ends = np.flatnonzero(seeds_right & (hl >= 0))
    if len(ends) == 0:
        return hl, hr, path, profile, info
    H = int(hl[ends].min())
    assert H == int(hr[seeds_left & (hr >= 0)].min())
    # the canonical path: back from the smallest-index right seed at H, every step to the smallest-index linked member one hop nearer
    path = np.empty(H + 1, dtype=np.int32)
    path[H] = ends[hl[ends] == H].min()
    for k in range(H, 0, -1):
        t = linked(ptr, nb, [path[k]])
        path[k - 1] = t[hl[t] == k - 1].min()
    # the corridor and its profile by hops_left
    rows = H + int(slack) + 1
    cor = np.flatnonzero((hl >= 0) & (hr >= 0) & (hl.astype(np.int64) + hr <= H + int(slack)))
    count = np.bincount(hl[cor], minlength=rows).astype(np.int32)
    xmin, xmax = np.full(rows, np.inf), np.full(rows, -np.inf)
    if x is not None:
        x = np.asarray(x, dtype=np.float64)
        np.minimum.at(xmin, hl[cor], x[cor]); np.maximum.at(xmax, hl[cor], x[cor])
    profile = dict(count=count, xmin=xmin, xmax=xmax)
    level = int(np.argmin(count[:H + 1]))                                   # the first of the smallest
    info.update(status=1, hops=H, corridor_sites=int(len(cor)), constriction_level=level, constriction_width=int(count[level]))
    return hl, hr, path, profile, info


def assert_equal(hops_left, hops_right, path, profile, info, ref):
    """Device result against analyse(): array_equal everywhere, doubles included."""
    rl, rr, rp, rprof, rinfo = ref
    assert np.array_equal(np.asarray(hops_left), rl)
    assert np.array_equal(np.asarray(hops_right), rr)
    assert np.asarray(path).dtype == np.int32 and np.array_equal(path, rp)
    for k in PROFILE:
        assert profile[k].dtype == rprof[k].dtype, k
        assert np.array_equal(profile[k], rprof[k]), k
    for k in INFO:
        assert info[k] == rinfo[k], (k, info[k], rinfo[k])


# ---- pinned cases (tests/test_path_ref.py, tests/test_gpu_paths.py) ----------------------------------------------------------------------
# the figures of the planted filaments of the two golden devices: the reference and the device are pinned to the same ones
PINNED_2P5_BRIDGED = {0: (2315, 19, 2), 2: (3123, 13, 3), 4: (3495, 13, 3)}            # slack: corridor sites, constriction level, width
PINNED_7P5_BRIDGED = {0: (3727, 13, 2), 2: (6849, 18, 2)}
