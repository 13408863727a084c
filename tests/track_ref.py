"""Host reference of the cluster tracking (dkmc_track_clusters; definitions: include/devicekmc_hip.h): two labellings of one device compared --
the per-site change codes, the distinct (prev, now) pairs in ascending first_site, one lineage row per component of either side, the transition
of the bridging verdict and the critical sites.  analyse() is numpy; brute() is the slow, obvious version (Python dicts over the sites) for small
N.  Everything they return is an integer or one of the input doubles, so the device result is compared with np.array_equal."""
import numpy as np

INFO = ("n_prev", "n_now", "n_pairs", "stayed", "joined", "left", "regrouped", "transition", "bridge_prev", "bridge_now",
        "born", "died", "merged", "split", "n_critical")
PAIRS = ("prev", "now", "count", "first_site")
NOW = ("root", "size", "joined", "n_parents", "main_parent", "flags")
PREV = ("root", "size", "left", "n_children", "main_child", "flags")
NONE, STAYED, JOINED, LEFT_, REGROUPED = 0, 1, 2, 3, 4                        # site_change
OPEN, CLOSED, RUPTURED, BRIDGED = 0, 1, 2, 3                                  # transition
TOUCH_LEFT, TOUCH_RIGHT = 1, 2
BORN, MERGED, FRAGMENT = 4, 8, 16                                             # now table
DIED, SPLIT, ABSORBED = 4, 8, 16                                              # prev table


def sides(label, N):
    label = np.asarray(label).astype(np.int64)
    return np.where((label >= 0) & (label < N), label, -1)


def _clamp(n, N):
    return min(max(int(n), 0), N)


def _i32(a):
    return np.asarray(a, dtype=np.int32).reshape(-1)


def _table(N, own, other, p_own, p_other, p_count, seeds):
    """One side's table from the pair rows.  own / other: the side ids per site; p_own / p_other / p_count: the pair rows seen from this side.
    -> (columns root, size, lone, links, main, contact bits; per-id arrays links_by_id, main_by_id)"""
    roots = np.unique(own[own >= 0])
    size = np.bincount(own[own >= 0], minlength=N)[roots]
    lone_by_id = np.zeros(N, dtype=np.int64)
    alone = (p_own >= 0) & (p_other < 0)
    lone_by_id[p_own[alone]] = p_count[alone]
    both = (p_own >= 0) & (p_other >= 0)
    links_by_id = np.bincount(p_own[both], minlength=N)
    main_by_id = np.full(N, -1, dtype=np.int64)
    order = np.lexsort((p_other[both], -p_count[both], p_own[both]))          # by own id, then the largest count, then the smallest other id
    o_own, o_other = p_own[both][order], p_other[both][order]
    head = np.r_[True, o_own[1:] != o_own[:-1]] if len(o_own) else np.zeros(0, dtype=bool)
    main_by_id[o_own[head]] = o_other[head]
    bits = np.zeros(N, dtype=np.int64)
    m = np.flatnonzero(own >= 0)
    np.bitwise_or.at(bits, own[m], seeds[m])
    return (roots, size, lone_by_id[roots], links_by_id[roots], main_by_id[roots], bits[roots]), links_by_id, main_by_id


def analyse(label_prev, label_now, x, n_left, n_right):
    """-> (site_change int32 [N], pairs, now, prev: dicts of int32 arrays, critical int32, info dict of INFO + critical_xmin / critical_xmax).
    x may be None: the x range is then +inf / -inf."""
    N = len(np.asarray(label_now))
    assert len(np.asarray(label_prev)) == N
    n_left, n_right = _clamp(n_left, N), _clamp(n_right, N)
    a, b = sides(label_prev, N), sides(label_now, N)
    site = np.arange(N)
    seeds = (site < n_left) * 1 + (site >= N - n_right) * 2
    # the pairs, in ascending first_site (np.unique reports the first occurrence)
    ids = np.flatnonzero((a >= 0) | (b >= 0))
    _, first, count = np.unique((a[ids] + 1) * (N + 1) + (b[ids] + 1), return_index=True, return_counts=True)
    order = np.argsort(ids[first])
    first_site, count = ids[first][order], count[order]
    pa, pb = a[first_site], b[first_site]
    pairs = dict(prev=_i32(pa), now=_i32(pb), count=_i32(count), first_site=_i32(first_site))
    (vr, vs, vl, vk, vm, vf), children_by_id, main_child = _table(N, a, b, pa, pb, count, seeds)
    (nr, ns, nl, nk, nm, nf), parents_by_id, main_parent = _table(N, b, a, pb, pa, count, seeds)
    vf = vf + DIED * (vk == 0) + SPLIT * (vk >= 2) + ABSORBED * ((vm >= 0) & (parents_by_id[np.maximum(vm, 0)] >= 2))
    nf = nf + BORN * (nk == 0) + MERGED * (nk >= 2) + FRAGMENT * ((nm >= 0) & (children_by_id[np.maximum(nm, 0)] >= 2))
    prev = dict(zip(PREV, (_i32(c) for c in (vr, vs, vl, vk, vm, vf))))
    now = dict(zip(NOW, (_i32(c) for c in (nr, ns, nl, nk, nm, nf))))
    # the per-site codes
    change = np.zeros(N, dtype=np.int32)
    change[(a < 0) & (b >= 0)] = JOINED
    change[(a >= 0) & (b < 0)] = LEFT_
    two = np.flatnonzero((a >= 0) & (b >= 0))
    on_main = (main_child[a[two]] == b[two]) & (main_parent[b[two]] == a[two])
    change[two] = np.where(on_main, STAYED, REGROUPED)
    # verdicts, critical sites
    bv, bn = vr[(vf & 3) == 3], nr[(nf & 3) == 3]
    bridge_prev, bridge_now = (int(bv.min()) if len(bv) else -1), (int(bn.min()) if len(bn) else -1)
    transition = (2 if bridge_prev >= 0 else 0) + (1 if bridge_now >= 0 else 0)
    if transition == CLOSED:
        critical = np.flatnonzero((b == bridge_now) & (a < 0))
    elif transition == RUPTURED:
        critical = np.flatnonzero((a == bridge_prev) & (b < 0))
    else:
        critical = np.zeros(0, dtype=np.int64)
    has_x = x is not None and len(critical) > 0
    xc = np.asarray(x, dtype=np.float64)[critical] if has_x else None
    info = dict(n_prev=len(vr), n_now=len(nr), n_pairs=len(first_site), stayed=len(two), joined=int((change == JOINED).sum()),
                left=int((change == LEFT_).sum()), regrouped=int((change == REGROUPED).sum()), transition=transition,
                bridge_prev=bridge_prev, bridge_now=bridge_now, born=int((nk == 0).sum()), died=int((vk == 0).sum()),
                merged=int((nk >= 2).sum()), split=int((vk >= 2).sum()), n_critical=len(critical),
                critical_xmin=float(xc.min()) if has_x else np.inf, critical_xmax=float(xc.max()) if has_x else -np.inf)
    return change, pairs, now, prev, _i32(critical), info


def brute(label_prev, label_now, x, n_left, n_right):
    """The same results from Python dicts over the sites, one definition at a time."""
    N = len(label_now)
    n_left, n_right = _clamp(n_left, N), _clamp(n_right, N)
    side = lambda v: int(v) if 0 <= int(v) < N else -1
    a, b = [side(v) for v in label_prev], [side(v) for v in label_now]
    count, first = {}, {}
    for i in range(N):
        if (a[i], b[i]) != (-1, -1):
            count[(a[i], b[i])] = count.get((a[i], b[i]), 0) + 1
            first.setdefault((a[i], b[i]), i)
    rows = sorted(count, key=lambda k: first[k])
    pairs = dict(prev=_i32([k[0] for k in rows]), now=_i32([k[1] for k in rows]), count=_i32([count[k] for k in rows]),
                 first_site=_i32([first[k] for k in rows]))

    def table(own, pick):
        """pick(pair) -> (own id, other id) of a pair"""
        out = {}
        for r in sorted(set(v for v in own if v >= 0)):
            members = [i for i in range(N) if own[i] == r]
            others = {pick(k)[1]: c for k, c in count.items() if pick(k)[0] == r and pick(k)[1] >= 0}
            lone = sum(c for k, c in count.items() if pick(k)[0] == r and pick(k)[1] < 0)
            main = min(others, key=lambda o: (-others[o], o)) if others else -1
            bits = (1 if any(i < n_left for i in members) else 0) | (2 if any(i >= N - n_right for i in members) else 0)
            out[r] = dict(root=r, size=len(members), lone=lone, links=len(others), main=main, flags=bits)
        return out

    P, Q = table(a, lambda k: (k[0], k[1])), table(b, lambda k: (k[1], k[0]))
    for r in P.values():
        r["flags"] |= (DIED if r["links"] == 0 else 0) | (SPLIT if r["links"] >= 2 else 0) | (ABSORBED if r["main"] >= 0 and Q[r["main"]]["links"] >= 2 else 0)
    for r in Q.values():
        r["flags"] |= (BORN if r["links"] == 0 else 0) | (MERGED if r["links"] >= 2 else 0) | (FRAGMENT if r["main"] >= 0 and P[r["main"]]["links"] >= 2 else 0)
    cols = ("root", "size", "lone", "links", "main", "flags")
    prev = {k: _i32([P[r][c] for r in sorted(P)]) for k, c in zip(PREV, cols)}
    now = {k: _i32([Q[r][c] for r in sorted(Q)]) for k, c in zip(NOW, cols)}
    change = np.zeros(N, dtype=np.int32)
    for i in range(N):
        if a[i] < 0 and b[i] < 0:
            change[i] = NONE
        elif a[i] < 0:
            change[i] = JOINED
        elif b[i] < 0:
            change[i] = LEFT_
        else:
            change[i] = STAYED if P[a[i]]["main"] == b[i] and Q[b[i]]["main"] == a[i] else REGROUPED
    bv = [r for r in sorted(P) if P[r]["flags"] & 3 == 3]
    bn = [r for r in sorted(Q) if Q[r]["flags"] & 3 == 3]
    bridge_prev, bridge_now = (bv[0] if bv else -1), (bn[0] if bn else -1)
    transition = {(False, False): OPEN, (False, True): CLOSED, (True, False): RUPTURED, (True, True): BRIDGED}[(bool(bv), bool(bn))]
    critical = []
    if transition == CLOSED:
        critical = [i for i in range(N) if b[i] == bridge_now and a[i] < 0]
    if transition == RUPTURED:
        critical = [i for i in range(N) if a[i] == bridge_prev and b[i] < 0]
    xs = [float(x[i]) for i in critical] if x is not None else []
    info = dict(n_prev=len(P), n_now=len(Q), n_pairs=len(rows), stayed=int(sum(c in (STAYED, REGROUPED) for c in change)),
                joined=int((change == JOINED).sum()), left=int((change == LEFT_).sum()), regrouped=int((change == REGROUPED).sum()),
                transition=transition, bridge_prev=bridge_prev, bridge_now=bridge_now,
                born=sum(1 for r in Q.values() if r["flags"] & BORN), died=sum(1 for r in P.values() if r["flags"] & DIED),
                merged=sum(1 for r in Q.values() if r["flags"] & MERGED), split=sum(1 for r in P.values() if r["flags"] & SPLIT),
                n_critical=len(critical), critical_xmin=min(xs) if xs else np.inf, critical_xmax=max(xs) if xs else -np.inf)
    return change, pairs, now, prev, _i32(critical), info


def assert_equal(change, pairs, now, prev, critical, info, ref):
    """A result (the device's, or brute()'s) against analyse(): array_equal on every column with the dtypes checked, doubles included."""
    rc, rp, rn, rv, rcrit, rinfo = ref
    change = np.asarray(change)
    assert change.dtype == np.int32 and np.array_equal(change, rc)
    for got, want, names in ((pairs, rp, PAIRS), (now, rn, NOW), (prev, rv, PREV)):
        assert tuple(got) == names
        for k in names:
            assert got[k].dtype == want[k].dtype == np.int32, k
            assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    assert np.asarray(critical).dtype == np.int32 and np.array_equal(critical, rcrit)
    for k in INFO + ("critical_xmin", "critical_xmax"):
        assert info[k] == rinfo[k], (k, info[k], rinfo[k])


# ---- cases (tests/test_track_ref.py, tests/test_gpu_track.py) ---------------------------------------------------------------------------
def random_pair(rng, N, k_prev, k_now, p_member=0.7):
    """two label arrays of N sites with at most k_prev / k_now distinct ids (drawn from 0 ... N - 1) and non-member values of every kind"""
    out = []
    for k in (k_prev, k_now):
        ids = rng.choice(N, size=min(k, N), replace=False)
        lab = ids[rng.integers(0, len(ids), N)].astype(np.int64)
        non = np.array([-1, N, N + 7, 2 ** 31 - 1, -2 ** 31], dtype=np.int64)
        out.append(np.where(rng.random(N) < p_member, lab, non[rng.integers(0, len(non), N)]).astype(np.int32))
    x = np.round(rng.normal(size=N) * 4.0) / 4.0                           # repeated values
    return out[0], out[1], x


def _rows(table, root):
    j = int(np.flatnonzero(table["root"] == root)[0])
    return {k: int(v[j]) for k, v in table.items()}


# ---- the 2.5 nm device: pristine, planted open (the filament without 25 < x < 40), planted full ---------------------------------------------
# per transition: info entries that are pinned
PINNED_2P5 = {
    ("pristine", "open"): dict(n_prev=79, n_now=70, n_pairs=81, stayed=3521, joined=60, left=0, merged=2, transition=0),
    ("open", "full"): dict(n_prev=70, n_now=65, n_pairs=71, joined=25, left=0, transition=1, bridge_prev=-1, bridge_now=0, n_critical=25),
    ("full", "open"): dict(n_prev=65, n_now=70, n_pairs=71, joined=0, left=25, transition=2, bridge_prev=0, bridge_now=-1, n_critical=25),
    ("open", "open"): dict(n_prev=70, n_now=70, n_pairs=70, joined=0, left=0, regrouped=0, merged=0, split=0, transition=0, n_critical=0),
}
PINNED_MEMBERS = dict(pristine=3521, open=3581, full=3606)
PLANTINGS = dict(pristine=None, open=(3.0, (25.0, 40.0)), full=(3.0, None))


def check_pinned_2p5(key, res):
    """the pinned figures of one transition on a result (change, pairs, now, prev, critical, info)"""
    change, pairs, now, prev, critical, info = res
    for k, v in PINNED_2P5[key].items():
        assert info[k] == v, (key, k, info[k], v)
    assert info["stayed"] + info["joined"] == PINNED_MEMBERS[key[1]] and info["stayed"] + info["left"] == PINNED_MEMBERS[key[0]], \
        (key, info["stayed"], info["joined"], info["left"], PINNED_MEMBERS)
    if key == ("open", "full"):
        assert _rows(now, 0)["n_parents"] == 6, (key, _rows(now, 0))
        assert abs(info["critical_xmin"] - 26.0348) <= 5e-5 and abs(info["critical_xmax"] - 39.945499) <= 5e-7, \
            (key, info["critical_xmin"], info["critical_xmax"])      # the printed digits
    if key == ("full", "open"):
        assert _rows(prev, 0)["n_children"] == 6, (key, _rows(prev, 0))
        assert abs(info["critical_xmin"] - 26.0348) <= 5e-5 and abs(info["critical_xmax"] - 39.945499) <= 5e-7, \
            (key, info["critical_xmin"], info["critical_xmax"])
    if key == ("open", "open"):
        assert not ((now["flags"] & MERGED) | (prev["flags"] & SPLIT)).any() and (change[change != 0] == STAYED).all(), \
            (key, now["flags"], prev["flags"], np.unique(change))
