"""Host reference of the min-cut analysis (dkmc_find_flow; definitions: include/devicekmc_hip.h): the largest family of conducting paths that
share no interior site (W), the minimum separators nearest either contact with their shores, and one canonical maximum family of strands, by
the synchronous search the header states, implemented literally -- breadth-first levels over the split nodes, the smallest exit, the smallest
predecessor at every step back --, with its rounds counted; plus a brute force over the subsets of the interior.  The search works on the members
only (frontiers, never whole-array sweeps per round).  Everything it returns is an integer or one of the input doubles, so the device result is
compared with np.array_equal."""
import itertools

import numpy as np

import path_ref as pr

INFO = ("status", "width", "left_shore", "right_shore", "shared_cut", "interior", "near_left", "near_right", "searches", "rounds",
        "longest_strand", "shortest_strand")
X4 = ("cut_left_xmin", "cut_left_xmax", "cut_right_xmin", "cut_right_xmax")
STRANDS = ("first_site", "last_site", "length", "offset", "left_seed", "right_seed", "cut_left_site", "cut_left_pos", "cut_right_site",
           "cut_right_pos")
ZONE = ("member", "left_shore", "left_cut", "right_cut", "right_shore")     # bit k of site_zone
MEMBER, LEFT_SHORE, LEFT_CUT, RIGHT_CUT, RIGHT_SHORE = 1, 2, 4, 8, 16
NONE, TERMINAL = -1, -2                                                     # pred / succ: no neighbour on a strand, the contact itself
BIG = 0x7fffffff


def graph(index, label, n_left, n_right):
    """-> (mask, ptr, nb, seeds_left, seeds_right): members, their links as rows in both directions, the clamped seeds"""
    label = np.asarray(label)
    N = len(label)
    n_left, n_right = min(max(int(n_left), 0), N), min(max(int(n_right), 0), N)
    mask = pr.member_mask(label, N)
    ids = np.arange(N)
    ptr, nb = pr.member_links(index, mask)
    return mask, ptr, nb, mask & (ids < n_left), mask & (ids >= N - n_right)


def _near(ptr, nb, seeds, interior):
    """the smallest seed linked to every interior site, BIG where there is none"""
    near = np.full(len(seeds), BIG, dtype=np.int64)
    s = np.flatnonzero(seeds)
    cnt = ptr[s + 1] - ptr[s]
    t = pr.linked(ptr, nb, s)
    np.minimum.at(near, t, np.repeat(s, cnt))
    near[~interior] = BIG
    return near


class _Search:
    """One breadth-first search of the model.  mirror = the same search on the mirrored problem (pred <-> succ, the near flags swapped; lin then
    holds the levels of the physical out-nodes).  Levels: -1 unlabelled; S has level 0; round k gives level k + 1."""

    def __init__(self, ptr, nb, interior, pred, succ, near_s, near_t, mirror=False, cap=None):
        if mirror:
            pred, succ = succ, pred
        N = len(interior)
        self.lin, self.lout = np.full(N, -1, dtype=np.int64), np.full(N, -1, dtype=np.int64)
        lin, lout = self.lin, self.lout
        self.end, self.capped = -1, False
        fin, fout = np.flatnonzero(near_s != BIG), np.zeros(0, dtype=np.int64)          # round 0: the arcs of S
        k = 0
        while True:
            if cap is not None and k >= cap:
                self.capped = True
                break
            if k > 0:
                # from the in-nodes at level k: the own out-node off a strand, the out-node of the strand predecessor on one
                a = fin[succ[fin] == NONE]
                b = pred[fin[succ[fin] != NONE]]
                nout = np.unique(np.concatenate([a, b[b >= 0]]))
                nout = nout[lout[nout] == -1]
                # from the out-nodes at level k: the own in-node on a strand, the in-node of every linked interior site but the successor
                a = fout[succ[fout] != NONE]
                cnt = ptr[fout + 1] - ptr[fout]
                t = pr.linked(ptr, nb, fout)
                t = t[interior[t] & (t != np.repeat(succ[fout], cnt))]
                nin = np.unique(np.concatenate([a, t]))
                nin = nin[lin[nin] == -1]
            else:
                nin, nout = fin, fout
            if len(nin) == 0 and len(nout) == 0:
                k += 1                                                      # the round that labels nothing is counted
                break
            lin[nin] = k + 1
            lout[nout] = k + 1
            exits = nout[(near_t[nout] != BIG) & (succ[nout] != TERMINAL)]
            k += 1
            if len(exits):
                self.end = int(exits.min())
                k += 1                                                      # the round that sees the exit word and returns is counted
                break
            fin, fout = nin, nout
        self.rounds = k
        self.capped = self.capped or (cap is not None and k > cap)          # the counted closing round is a round too


def _augment(ptr, nb, interior, pred, succ, s):
    """Walks back from the end node of a successful search, the smallest predecessor one level lower at every node, and flips the path.
    -> True if the path used an arc that cancels flow."""
    lin, lout = s.lin, s.lout
    cur, out, lev = s.end, True, int(s.lout[s.end])
    nxt = None                                                              # the node after cur on the path: None = the right contact
    backward = False
    while True:
        if out:
            v = cur
            y = v if succ[v] == NONE else int(succ[v])                      # the in-node of v itself, or of its successor (cancelling v -> y)
            assert lin[y] == lev - 1
            if nxt is None:
                succ[v] = TERMINAL
            elif nxt != v:
                succ[v] = nxt
                pred[nxt] = v
            else:
                backward = True                                             # v_out -> v_in: the flow through v is cancelled
        else:
            w = cur
            if nxt != w:                                                    # w_in -> u_out: cancels u -> w
                backward = True
                if succ[nxt] == w:
                    succ[nxt] = NONE
                if pred[w] == nxt:
                    pred[w] = NONE
            if lev == 1:
                pred[w] = TERMINAL
                return backward
            t = nb[ptr[w]:ptr[w + 1]]
            t = t[interior[t] & (lout[t] == lev - 1) & (succ[t] != w) & (t != w)]
            cand = [int(t.min())] if len(t) else []
            if succ[w] != NONE and lout[w] == lev - 1:
                cand.append(w)
            y = min(cand)
        nxt, cur, out, lev = cur, y, not out, lev - 1


def analyse(index, label, x, n_left, n_right, max_strands=64, cap=None, trace=None):
    """-> (site_zone int32 [N], site_strand int32 [N], strand table dict of STRANDS (int32), strand sites int32, info dict of INFO + X4).
    x may be None: the x entries then hold +inf / -inf.  cap: the round cap of one search (None: none); a search that reaches it raises
    OverflowError.  trace: a dict that receives backward = the number of searches whose path cancelled flow."""
    assert 1 <= int(max_strands) <= 4096
    mask, ptr, nb, seeds_left, seeds_right = graph(index, label, n_left, n_right)
    N = len(mask)
    interior = mask & ~seeds_left & ~seeds_right
    zone = mask.astype(np.int32) * MEMBER
    strand = np.full(N, -1, dtype=np.int32)
    table = dict((k, np.zeros(0, dtype=np.int32)) for k in STRANDS)
    info = dict((k, 0) for k in INFO)
    info.update(cut_left_xmin=np.inf, cut_left_xmax=-np.inf, cut_right_xmin=np.inf, cut_right_xmax=-np.inf)
    if N == 0:
        return zone, strand, table, np.zeros(0, dtype=np.int32), info
    near_l, near_r = _near(ptr, nb, seeds_left, interior), _near(ptr, nb, seeds_right, interior)
    info.update(interior=int(interior.sum()), near_left=int((near_l != BIG).sum()), near_right=int((near_r != BIG).sum()))
    touch = bool((seeds_left & seeds_right).any()) or bool(seeds_right[pr.linked(ptr, nb, np.flatnonzero(seeds_left))].any())
    if touch:
        info.update(status=2, width=-1)
        return zone, strand, table, np.zeros(0, dtype=np.int32), info
    pred, succ = np.full(N, NONE, dtype=np.int64), np.full(N, NONE, dtype=np.int64)
    W = searches = rounds = n_backward = 0
    status = None
    while status is None:
        s = _Search(ptr, nb, interior, pred, succ, near_l, near_r, cap=cap)
        if s.capped:
            raise OverflowError("search not finished after %d rounds" % cap)
        searches += 1
        rounds += s.rounds
        if s.end < 0:
            status = 1 if W else 0
        else:
            n_backward += bool(_augment(ptr, nb, interior, pred, succ, s))
            W += 1
            if W == int(max_strands):
                status = 3
    if trace is not None:
        trace["backward"] = n_backward
    info.update(status=status, width=W, searches=searches, rounds=rounds)
    if status != 3:
        m = _Search(ptr, nb, interior, pred, succ, near_r, near_l, mirror=True, cap=cap)
        if m.capped:
            raise OverflowError("search not finished after %d rounds" % cap)
        info["searches"] += 1
        info["rounds"] += m.rounds
        shore_l, shore_r = seeds_left | (s.lout >= 0), seeds_right | (m.lout >= 0)
        cut_l, cut_r = (s.lin >= 0) & (s.lout < 0), (m.lin >= 0) & (m.lout < 0)
        zone += shore_l * LEFT_SHORE + cut_l * LEFT_CUT + cut_r * RIGHT_CUT + shore_r * RIGHT_SHORE
        info.update(left_shore=int(shore_l.sum()), right_shore=int(shore_r.sum()), shared_cut=int((cut_l & cut_r).sum()))
        if x is not None:
            x = np.asarray(x, dtype=np.float64)
            if cut_l.any():
                info.update(cut_left_xmin=x[cut_l].min(), cut_left_xmax=x[cut_l].max())
            if cut_r.any():
                info.update(cut_right_xmin=x[cut_r].min(), cut_right_xmax=x[cut_r].max())
    # the strands, in ascending first site
    firsts = np.flatnonzero(pred == TERMINAL)
    assert len(firsts) == W
    cols = dict((k, np.full(W, -1, dtype=np.int32)) for k in STRANDS)
    sites = []
    for j, f in enumerate(firsts):
        cols["first_site"][j], cols["offset"][j], cols["left_seed"][j] = f, len(sites), near_l[f]
        v, n = int(f), 0
        while True:
            sites.append(v)
            strand[v] = j
            if status != 3 and zone[v] & LEFT_CUT:
                cols["cut_left_site"][j], cols["cut_left_pos"][j] = v, n
            if status != 3 and zone[v] & RIGHT_CUT:
                cols["cut_right_site"][j], cols["cut_right_pos"][j] = v, n
            n += 1
            if succ[v] == TERMINAL:
                break
            v = int(succ[v])
        cols["last_site"][j], cols["length"][j], cols["right_seed"][j] = v, n, near_r[v]
    if W:
        info.update(longest_strand=int(cols["length"].max()), shortest_strand=int(cols["length"].min()))
    return zone, strand, cols, np.array(sites, dtype=np.int32), info


def connected(ptr, nb, seeds_left, seeds_right, alive):
    """-> (some left seed reaches a right seed over the sites of alive, the sites reached from the left seeds)"""
    seen = seeds_left & alive
    front = np.flatnonzero(seen)
    while len(front):
        t = np.unique(pr.linked(ptr, nb, front))
        t = t[alive[t] & ~seen[t]]
        seen[t] = True
        front = t
    return bool((seen & seeds_right).any()), seen


def brute_width(index, label, n_left, n_right, all_minimum=False):
    """The definition itself: the subsets of the interior in order of size; W = the size of the first whose deletion leaves no left seed
    connected to a right seed (-1 when the contacts touch).  all_minimum: -> (W, [(separator tuple, left shore mask)] of every separator of
    that size)."""
    mask, ptr, nb, seeds_left, seeds_right = graph(index, label, n_left, n_right)
    interior = np.flatnonzero(mask & ~seeds_left & ~seeds_right)
    if connected(ptr, nb, seeds_left, seeds_right, mask & (seeds_left | seeds_right))[0]:
        return (-1, []) if all_minimum else -1                             # the contacts touch: no deletion of interior sites separates them
    found = []
    for size in range(len(interior) + 1):
        for sub in itertools.combinations(interior.tolist(), size):
            alive = mask.copy()
            alive[list(sub)] = False
            hit, seen = connected(ptr, nb, seeds_left, seeds_right, alive)
            if not hit:
                if not all_minimum:
                    return size
                found.append((sub, seen | seeds_left))
        if found:
            return size, found
    return (-1, []) if all_minimum else -1


def assert_equal(zone, strand, table, sites, info, ref, rows=None):
    """Device result against analyse(): array_equal everywhere, doubles included."""
    r_zone, r_strand, r_table, r_sites, r_info = ref
    assert np.asarray(zone).dtype == np.int32 and np.array_equal(np.asarray(zone), r_zone)
    assert np.asarray(strand).dtype == np.int32 and np.array_equal(np.asarray(strand), r_strand)
    for k in STRANDS:
        n = len(r_table[k]) if rows is None else min(rows, len(r_table[k]))
        assert table[k].dtype == np.int32, k
        assert np.array_equal(table[k], r_table[k][:n]), k
    assert np.asarray(sites).dtype == np.int32 and np.array_equal(sites, r_sites)
    for k in INFO:
        assert info[k] == r_info[k], (k, info[k], r_info[k])
    for k in X4:
        assert np.array_equal(np.float64(info[k]), np.float64(r_info[k])), (k, info[k], r_info[k])


# ---- pinned cases and their graphs (tests/test_flow_ref.py, tests/test_gpu_flow.py) -------------------------------------------------------
def rails(k, length, rng=None):
    """k rails of `length` sites with a rung between neighbouring rails at every level: site k i + j is rail j at level i; with rng the sites of
    every level are renumbered at random, so that the rails swap site numbers"""
    site = np.arange(k * length).reshape(length, k)
    if rng is not None:
        site = np.stack([rng.permutation(row) for row in site])
    links = [(site[i, j], site[i + 1, j]) for i in range(length - 1) for j in range(k)]
    links += [(site[i, j], site[i, j + 1]) for i in range(length) for j in range(k - 1)]
    return links


# radius: W, the left-most minimum cut, the right-most one of the planted filaments of the 2.5 nm golden device
PINNED_2P5 = {3.0: (2, [2792, 2864], [2972, 3014]), 2.6: (1, [1776], [1776]), 2.4: (1, [1776], [2010]), 2.2: (1, [1776], [4414]),
              4.5: (6, [1337, 1375, 1468, 1469, 1492, 1511], [4354, 4380, 4401, 4414, 4464, 4517])}
PINNED_2P5_ROUNDS = {3.0: (4, 296), 2.6: (3, 195), 2.4: (3, 193), 2.2: (3, 155), 4.5: (8, 610)}            # searches, rounds
