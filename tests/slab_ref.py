"""numpy restatement of the slab partition (csrc/slab.h), from the comments of its kernels -- the reference of tests/test_gpu_slab_plan.py.

Rows [first, m) of a symmetric pattern are distributed; coord[i] is the lateral coordinate of row first + i.
  u      = (x - lo) / (hi - lo), or 0 when hi <= lo
  bin    = trunc(4096 u), clamped to 0 ... 4095
  cuts[r] = the first bin with at least r / nr of the rows strictly below it (4096 when there is none)
  owner  = the number of cuts r >= 1 at or below the row's bin; 0 for the rows < first
  mask   bit d of a row >= first: the row has an entry in a row >= first owned by d != its own owner; bit 31 of a column word is masked off
  tab    = rows per owner | rows with mark >= 0 per owner | hal[s * nr + d] = rows of s with bit d
  lists  ascending: rows_by_owner grouped by owner; what v sends = its rows with bit d, d ascending, d != v; what v receives = the rows of s with
         bit v, s ascending, s != v
The cases use integer-valued coordinates whose bins are not integers' neighbours: no bin depends on a rounding."""
import numpy as np

BINS = 4096


def bins(coord, lo, hi):
    coord = np.asarray(coord, dtype=np.float64)
    u = (coord - lo) / (hi - lo) if hi > lo else np.zeros_like(coord)
    return np.clip(np.trunc(BINS * u), 0, BINS - 1).astype(np.int64)


def cuts(b, nr):
    hist = np.bincount(b, minlength=BINS)
    below = np.concatenate(([0], np.cumsum(hist)))[:BINS]             # rows strictly below bin b
    out = np.full(nr + 1, BINS, dtype=np.int64)
    out[0] = 0
    for r in range(1, nr):
        hit = np.nonzero(below * nr >= r * len(b))[0]
        if len(hit):
            out[r] = hit[0]
    return out


def partition(m, first, rp, ci, coord, lo, hi, nr, mark=None):
    """dict(owner, mask, tab, rows_by_owner, nown, nmark, hal)"""
    rp, ci = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64)
    b = bins(coord, lo, hi)
    cu = cuts(b, nr)
    owner = np.zeros(m, dtype=np.int64)
    owner[first:] = (cu[1:nr][None, :] <= b[:, None]).sum(axis=1)
    rows = np.repeat(np.arange(m), np.diff(rp))
    cols = ci & 0x7fffffff
    use = (rows >= first) & (cols >= first)
    use[use] = owner[cols[use]] != owner[rows[use]]
    mask = np.zeros(m, dtype=np.uint32)
    np.bitwise_or.at(mask, rows[use], (np.uint32(1) << owner[cols[use]].astype(np.uint32)))
    nown = np.bincount(owner[first:], minlength=nr)
    marked = np.ones(m - first, dtype=bool) if mark is None else np.asarray(mark)[first:] >= 0
    nmark = np.zeros(nr, dtype=np.int64) if mark is None else np.bincount(owner[first:][marked], minlength=nr)
    hal = np.zeros((nr, nr), dtype=np.int64)
    for d in range(nr):
        hal[:, d] = np.bincount(owner[first:][(mask[first:] >> np.uint32(d)) & np.uint32(1) == 1], minlength=nr)
    rows_by_owner = first + np.argsort(owner[first:], kind="stable")
    return dict(owner=owner, mask=mask, nown=nown, nmark=nmark, hal=hal, tab=np.concatenate((nown, nmark, hal.reshape(-1))), rows_by_owner=rows_by_owner)


def halo_lists(part, first, nr, v):
    """(hsend, hrecv) of rank v"""
    owner, mask = part["owner"], part["mask"]
    idx = np.arange(first, len(owner))

    def rows(s, bit):
        return idx[(owner[first:] == s) & ((mask[first:] >> np.uint32(bit)) & np.uint32(1) == 1)]
    send = [rows(v, d) for d in range(nr) if d != v]
    recv = [rows(s, v) for s in range(nr) if s != v]
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    return cat(send), cat(recv)


def csr(m, links, diagonal=True):
    """symmetric CSR pattern of the undirected links (i, j), columns ascending"""
    adj = [set([i]) if diagonal else set() for i in range(m)]
    for i, j in links:
        adj[i].add(j); adj[j].add(i)
    rp = np.zeros(m + 1, dtype=np.int32)
    rp[1:] = np.cumsum([len(a) for a in adj])
    ci = np.array([c for a in adj for c in sorted(a)], dtype=np.int32)
    return rp, ci


def chain_csr(m, first=0):
    """rows first ... m - 1 linked in a chain, with the diagonal; vectorised (the large case)"""
    n = m - first
    cnt = np.full(n, 3, dtype=np.int64); cnt[0] -= 1; cnt[-1] -= 1
    if n == 1:
        cnt[0] = 1
    rp = np.zeros(m + 1, dtype=np.int32)
    rp[first + 1:] = np.cumsum(cnt)
    i = np.repeat(np.arange(first, m), 3).reshape(n, 3) + np.array([-1, 0, 1])
    keep = (i >= first) & (i < m)
    return rp, i[keep].astype(np.int32)


def cases():
    """name -> dict(m, first, rp, ci, coord, lo, hi, nr, mark)"""
    out = {}
    c12 = np.arange(12, dtype=np.float64)
    chain12 = [(i, i + 1) for i in range(11)]
    rp, ci = csr(12, chain12)
    out["a_chain_one_rank"] = dict(m=12, first=0, rp=rp, ci=ci, coord=c12, lo=0.0, hi=11.0, nr=1, mark=None)
    rp, ci = csr(12, chain12 + [(0, 11)])
    out["b_ring_three_ranks"] = dict(m=12, first=0, rp=rp, ci=ci, coord=c12, lo=0.0, hi=11.0, nr=3, mark=None)
    # c: rows 0 / 1 are driver rows with entries in every row; rows 2 ... 13 form a chain and link to columns 0 and 1
    links = [(i, i + 1) for i in range(2, 13)] + [(0, j) for j in range(2, 14)] + [(1, j) for j in range(2, 14)] + [(0, 1)]
    rp, ci = csr(14, links)
    mark = np.array([5, 6] + [(-1 if i % 3 else i) for i in range(12)], dtype=np.int32)      # -1 on two rows in three; the driver rows carry marks that must not count
    out["c_driver_rows_and_marks"] = dict(m=14, first=2, rp=rp, ci=ci, coord=c12, lo=0.0, hi=11.0, nr=3, mark=mark)
    rp, ci = csr(12, chain12)
    out["d_all_in_one_bin"] = dict(m=12, first=0, rp=rp, ci=ci, coord=np.full(12, 7.0), lo=7.0, hi=7.0, nr=3, mark=None)
    rp, ci = csr(40, [(i, i + 1) for i in range(39)])
    out["e_thirty_two_ranks"] = dict(m=40, first=0, rp=rp, ci=ci, coord=np.arange(40, dtype=np.float64), lo=0.0, hi=39.0, nr=32, mark=None)
    b = out["b_ring_three_ranks"]
    ci31 = b["ci"].copy(); ci31[1::2] |= np.int32(-2 ** 31)
    out["f_class_bit_31"] = dict(b, ci=ci31)
    rp, ci = csr(10, [(i, i + 1) for i in range(9)])
    out["g_heavy_bin_empty_slab"] = dict(m=10, first=0, rp=rp, ci=ci, coord=np.array([0, 1, 2, 4, 4, 4, 4, 4, 4, 9], dtype=np.float64), lo=0.0, hi=9.0, nr=4, mark=None)
    out["h_clamped_ends"] = dict(m=10, first=0, rp=rp, ci=ci, coord=np.array([-5, -3, -1, 0, 1, 8, 9, 10, 12, 20], dtype=np.float64), lo=0.0, hi=10.0, nr=2, mark=None)
    n = 140000
    rp, ci = chain_csr(n)
    out["i_large_chain"] = dict(m=n, first=0, rp=rp, ci=ci, coord=np.arange(n, dtype=np.float64), lo=0.0, hi=float(n - 1), nr=5, mark=None)
    return out
