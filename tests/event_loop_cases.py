"""Synthetic inputs of the event-loop tests (tests/test_event_loop_ref.py, tests/test_gpu_event_loop.py): symmetric indexes padded with -1, tables
with exact sums, and draws chosen event by event from the state of the reference (tests/event_loop_ref.py).  No GPU, no file access."""
import functools

import numpy as np

import event_loop_ref as ref

SCALE = 2.0 ** -20          # one table unit, in 1 / s
N_TARGET = 70               # events a case asks for; every event retires two sites, so small or dense shapes run dry before


def ring_index(N, rng):
    """nn = 2: a ring over a random relabelling of the sites, the two neighbours of a row in random order.  Symmetric by construction."""
    perm = rng.permutation(N)
    neigh = np.empty((N, 2), dtype=np.int32)
    neigh[perm, 0] = np.roll(perm, 1); neigh[perm, 1] = np.roll(perm, -1)
    swap = rng.random(N) < 0.5
    neigh[swap] = neigh[swap][:, ::-1]
    return neigh.reshape(-1)


def graph_index(N, nn, rng, p_edge):
    """A random undirected graph of degree <= nn without self-loops or duplicates; the neighbours of a row at random positions, pads -1."""
    adj = [[] for _ in range(N)]
    iu, ju = np.triu_indices(N, 1)
    order = rng.permutation(len(iu))
    keep = rng.random(len(iu)) < p_edge
    for q in order[keep[order]]:
        a, b = int(iu[q]), int(ju[q])
        if len(adj[a]) < nn and len(adj[b]) < nn:
            adj[a].append(b); adj[b].append(a)
    neigh = np.full((N, nn), -1, dtype=np.int32)
    for a in range(N):
        pos = rng.permutation(nn)[:len(adj[a])]
        neigh[a, pos] = rng.permutation(adj[a])
    return neigh.reshape(-1)


def check_index(neigh, N, nn):
    """The contract of the loop: entries in [-1, N), no self-loops, no duplicates, symmetric."""
    neigh = np.asarray(neigh).reshape(N, nn)
    assert neigh.min() >= -1 and neigh.max() < N
    rows = np.repeat(np.arange(N), nn)[neigh.reshape(-1) >= 0]
    cols = neigh.reshape(-1)[neigh.reshape(-1) >= 0].astype(np.int64)
    assert (rows != cols).all()
    fwd = np.sort(rows * N + cols); back = np.sort(cols * N + rows)
    assert len(np.unique(fwd)) == len(fwd) and np.array_equal(fwd, back)


def exact_table(neigh, rng, smax=20):
    """Rates k 2^s in table units, k in 1 ... 1023, s in 0 ... smax; zero in about a third of the live slots and in every pad."""
    n = len(neigh)
    t = rng.integers(1, 1024, n).astype(np.int64) << rng.integers(0, smax + 1, n).astype(np.int64)
    t[rng.random(n) < 1 / 3] = 0
    t[neigh < 0] = 0
    if t.sum() == 0:
        t[np.flatnonzero(neigh >= 0)[0]] = 3 << 7
    assert float(t.sum()) < 2.0 ** 52
    return t


def _edge_draw(E, Psum):
    """u with u * Psum == E in one double multiplication, or None (about one wanted edge in ten has none)."""
    u0 = np.float64(E) / np.float64(Psum)
    for u in (u0, np.nextafter(u0, 0.0), np.nextafter(u0, 1.0)):
        if 0.0 <= u < 1.0 and u * np.float64(Psum) == np.float64(E):
            return float(u)
    return None


class Case:
    pass


MENU = ("edge", "below", "zero", "top", "random")


@functools.lru_cache(maxsize=None)
def build_case(N, nn, seed, p_edge=0.5, weights=(0.5, 0.15, 0.05, 0.05, 0.25), one_at=1, n_target=N_TARGET):
    """One table, index, state and list of draws.  The draws are chosen per event from the reference's own state:
    edge   -- the lower edge of a live bucket exactly (accepted only if u * Psum == edge in Python; otherwise the event draws at random),
    below  -- the largest u whose number lies below such an edge,
    zero   -- 0.0;  top -- 1 - 2^-53;  random -- uniform;  one -- 1.0, once, at event `one_at` (the fallback branch),
    and, where rows >= 262 144 exist, event 0 aims at the middle of a bucket there.  The waiting-time draw of every event but the last asked for gives
    dt = 1 / (4 freq), the last one 4 / freq, so that no stop decision rests on the last bits of log()."""
    rng = np.random.default_rng(1000003 * seed + 1000 * N + nn)
    c = Case()
    c.N, c.nn, c.seed = N, nn, seed
    c.neigh = ring_index(N, rng) if nn == 2 and N >= 3 else graph_index(N, nn, rng, p_edge)
    check_index(c.neigh, N, nn)
    c.table = exact_table(c.neigh, rng)
    if N > 262144:
        c.table[262144 * nn] = 517 << 9                     # a live slot in the only row of the top level's second chunk
    c.element = rng.integers(0, 5, N).astype(np.int32)
    c.charge = rng.integers(-2, 3, N).astype(np.int32)
    c.freq = float(c.table.sum()) * SCALE / 16
    lp = ref.EventLoop(c.table, c.neigh, c.element, c.charge, c.freq, SCALE)
    draws, kinds, n_edge = [], [], 0
    for ev in range(n_target):
        Psum = lp.psum
        if Psum == 0:
            break
        cum = lp.prefix()
        live = np.flatnonzero(lp.P > 0)
        kind = "one" if ev == one_at else "high" if (ev == 0 and N > 262144) else MENU[rng.choice(5, p=weights)]
        if kind in ("edge", "below"):
            u = None
            for _ in range(8):
                if len(live) < 2:
                    break
                cand = live[1:]
                if nn > 64 and rng.random() < 0.4 and (cand % nn >= 64).any():
                    cand = cand[cand % nn >= 64]                # a bucket in the second 64-slot chunk of its row
                k = int(cand[rng.integers(len(cand))])
                E = int(cum[k - 1])
                u = _edge_draw(E, Psum)
                if u is not None:
                    break
            if u is None:
                kind = "random"
            elif kind == "below":
                while u * np.float64(Psum) >= np.float64(E):
                    u = float(np.nextafter(u, 0.0))
            else:
                n_edge += 1
        if kind == "high":
            k = int(live[live >= 262144 * nn][0])
            u = (float(cum[k]) - float(lp.P[k]) / 2) / float(Psum)
        elif kind == "zero":
            u = 0.0
        elif kind == "top":
            u = 1.0 - 2.0 ** -53
        elif kind == "one":
            u = 1.0
        elif kind == "random":
            u = float(rng.random())
        x = float(Psum) * SCALE / c.freq
        last = ev == n_target - 1
        u2 = float(np.exp(-(4.0 if last else 0.25) * x))
        dt = lp.step(u, u2)
        assert dt >= 2 / c.freq if last else dt <= 0.5 / c.freq, (ev, dt, c.freq)
        draws += [u, u2]; kinds.append(kind)
    draws += [0.5, 0.5]                                         # never the reason to stop: the table is dry or the last dt has ended the step
    c.draws = np.array(draws, dtype=np.float64)
    c.kinds, c.n_edge = kinds, n_edge
    c.ref = ref.run(c.table, c.neigh, c.element, c.charge, c.freq, c.draws, SCALE)
    assert c.ref["n_events"] == len(kinds) and not c.ref["exhausted"] and c.ref["dry"] == (len(kinds) < n_target)
    assert [tuple(r) for r in c.ref["log"]] == lp.log
    return c
