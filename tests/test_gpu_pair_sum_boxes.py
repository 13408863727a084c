"""The screened pair sum (dkmc_poisson_gridless_gpu, csrc/potential.hip) on small synthetic boxes against the extended-precision reference of
tests/pair_sum_ref.py (pinned by tests/test_pair_sum_ref.py): raw device pointers, no Device, no structure file.  The boxes reach what the shipped
cell and its square tilings never do -- ny != nz, narrow and clamped axes, all 32 x 32 columns, empty columns, sites outside the box and on cell
faces, 1 and 16 x bins, a segment above PW_SORTCAP, the ncharged = 512 switch between the two kernels, a box changed behind unchanged pointers.

Per case and pbc: all pairs (cut-off 0) within 1e-12 of the largest potential and N nq - nq pairs evaluated; with the cut-off at 6.5 the kernel the
case names, EXACTLY the reference's number of pairs inside the cut-off, 0.0 where a site has none, every other site within 1e-12 of its own sum
of magnitudes of the in-range sum (rounding of eight interleaved partial sums of <= 2 000 terms stays below 6e-14 of it; one lost, doubled or
wrongly imaged term above 1e-12 of the site's sum breaks it); a second run and form 1 bit for bit with equal counters.

Largest measured |got - v_in| / abs_in over all cases on an MI355X: 5.4e-14 (`outside`, pbc 1; consistent with a site whose few in-range
neighbours all lie near the cut-off, where one rounding of erfc's argument is worth 2 x 6.5^2 = 85 of the term); 2e-15 ... 3e-14 on the other
cases.  -s prints the figure of every case.

That the cases discriminate was checked once by hand against three wrong builds: `c % G.nz` for `c % G.ny` in k_pairwise_cells fails every case
with ny != nz and a windowed y axis (all but rect_T, both_narrow, full_grid) and `bhi` for `bhi + 1` fails every case that takes the cell list,
both on the exact pair count; pw_d2 without the round() of fz fails every pbc run, on the all-pairs potentials."""
import ctypes as C

import numpy as np
import pytest

import pair_sum_ref as R

pytestmark = pytest.mark.gpu

UNWRITTEN = 1.0e30         # what the output holds before a call: no potential, and finite (freed device memory keeps it; an export elsewhere in the suite reads unwritten memory)


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__ as g
    g.build()
    import torch
    from devicekmc_amd import host, lib
    L = lib.load()
    host._use_stream(torch.device("cuda:0"))
    return host, L


def _restore(L):
    L.dkmc_set_pair_form(0); L.dkmc_set_pair_cutoff(6.5); L.dkmc_set_profiling(0)
    L.dkmc_reset_pair_sum_cache()


class Box:
    """The device arrays of one case: made once, so that every call of a test passes the same pointers."""

    def __init__(self, c, q):
        import torch
        dev = torch.device("cuda:0")
        up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(dev)
        self.N = c.N
        self.x, self.y, self.z = up(c.x, np.float64), up(c.y, np.float64), up(c.z, np.float64)
        self.lattice, self.sigma, self.k = up(c.lattice, np.float64), up([c.sigma], np.float64), up([R.K], np.float64)
        self.q = up(q, np.int32)
        self.out = torch.empty(c.N, dtype=torch.float64, device=dev)


def _sum(hip, b, pbc, form, cut):
    """One profiled pair sum: (potentials, pair_evaluated, pair_tested, cell list used)."""
    import torch
    from devicekmc_amd.host import _ptr
    from devicekmc_amd.lib import check
    host, L = hip
    L.dkmc_set_pair_form(form); L.dkmc_set_pair_cutoff(cut); L.dkmc_set_profiling(1)
    b.out.fill_(UNWRITTEN)
    check(L.dkmc_poisson_gridless_gpu(0, int(pbc), b.N, _ptr(b.lattice), _ptr(b.sigma), _ptr(b.k), _ptr(b.x), _ptr(b.y), _ptr(b.z), _ptr(b.q), _ptr(b.out)))
    torch.cuda.synchronize()
    st = host.get_stats()
    info, ms = (C.c_longlong * 6)(), (C.c_double * 2)()
    check(L.dkmc_get_pair_sum_info(info, ms))
    assert info[0] == form
    return b.out.cpu().numpy().copy(), st["pair_evaluated"], st["pair_tested"], int(info[1])


def _check_cut(got, ev, te, used, ref, use, what):
    """The assertions on one call with the cut-off on; returns the largest |got - v_in| / abs_in."""
    assert used == use, (what, used)
    assert ev == int(ref.n_in.sum()), (what, ev, int(ref.n_in.sum()))
    assert te >= ev, (what, te, ev)
    none = ref.n_in == 0
    assert np.isfinite(got).all(), what
    assert not got[none].any(), (what, np.flatnonzero(none & (got != 0.0))[:8])
    err = np.abs(got.astype(R.LD) - ref.v_in)
    bad = np.flatnonzero(err > R.LD(1e-12) * ref.abs_in)
    assert bad.size == 0, (what, bad[:8], [float(err[i] / ref.abs_in[i]) for i in bad[:8]])
    scale = np.abs(ref.v_all).max()
    assert np.abs(got.astype(R.LD) - ref.v_all).max() <= R.LD(1e-12) * scale, what
    return float((err[~none] / ref.abs_in[~none]).max()) if (~none).any() else 0.0


def _check_all(got, ev, te, ref, N, nq, what):
    scale = np.abs(ref.v_all).max()
    assert np.isfinite(got).all(), what
    assert np.abs(got.astype(R.LD) - ref.v_all).max() <= R.LD(1e-12) * scale, (what, float(np.abs(got.astype(R.LD) - ref.v_all).max() / scale))
    assert ev == N * nq - nq and te == N * nq, (what, ev, te)


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]), (what, float(np.abs(a[0] - b[0]).max()))
    assert a[1:] == b[1:], (what, a[1:], b[1:])


def _step(hip, b, c, pbc, ref, use, what, reset):
    """Everything one (case, pbc, charge vector) must meet.  With `reset` the cached grouping is dropped first; without it the calls run on whatever
    the previous step left."""
    host, L = hip
    nq = int(np.count_nonzero(b.q.cpu().numpy()))
    def all_pairs():
        a0 = _sum(hip, b, pbc, 0, 0.0)
        _check_all(a0[0], a0[1], a0[2], ref, c.N, nq, what + ", all pairs")
        _same(a0, _sum(hip, b, pbc, 1, 0.0), what + ", form 1, all pairs")

    if reset:
        L.dkmc_reset_pair_sum_cache()
        all_pairs()
    c0 = _sum(hip, b, pbc, 0, R.XCUT)
    worst = _check_cut(*c0, ref, use, what)
    if c.tested_below:
        assert c0[2] < c.tested_below * c.N * nq, (what, c0[2] / (c.N * nq))
    _same(c0, _sum(hip, b, pbc, 0, R.XCUT), what + ", second run")
    _same(c0, _sum(hip, b, pbc, 1, R.XCUT), what + ", form 1")
    all_pairs()                                                         # (another cut-off is another key: without `reset` the calls above ran on the kept grouping; the one below regroups)
    _same(c0, _sum(hip, b, pbc, 0, R.XCUT), what + ", after the all-pairs calls")
    print("%s: %d sites, %d charged, kernel %d, %d pairs inside the cut-off of %d tested (%.3f of N nq); max |got - v_in| / abs_in = %.3e"
          % (what, c.N, nq, c0[3], c0[1], c0[2], c0[2] / (c.N * nq), worst))
    return c0[0]


@pytest.mark.parametrize("name,pbc", R.RUNS)
def test_pair_sum_on_a_box(hip, name, pbc):
    host, L = hip
    c = R.case(name)
    b = Box(c, c.steps[0].q)
    try:
        for k, s in enumerate(c.steps):
            if k:
                import torch
                b.q.copy_(torch.as_tensor(s.q))                         # in place: the same pointers, the same cached grouping, no reset
            got = _step(hip, b, c, pbc, R.reference(name, pbc, k), s.grid[5], "%s pbc %d step %d" % (name, pbc, k), reset=k == 0)
        if c.same_as:                                                   # y and z swapped: the potentials of the other case, site by site
            other = R.reference(c.same_as, pbc)
            err = np.abs(got.astype(R.LD) - other.v_in)
            assert (err <= R.LD(1e-12) * other.abs_in).all() and np.abs(got.astype(R.LD) - other.v_all).max() <= R.LD(1e-12) * np.abs(other.v_all).max()
    finally:
        _restore(L)


def test_box_changed_in_place(hip):
    """lattice[1] grows by half behind the same pointers, no reset: the device sees the other box (PwGrid::rebuild), regroups the sites into its
    19 x 5 columns and, with pbc, images through the new face."""
    host, L = hip
    c = R.case("rect")
    q = c.steps[0].q
    for pbc in (0, 1):
        b = Box(c, q)
        try:
            _step(hip, b, c, pbc, R.reference("rect", pbc), 1, "rect pbc %d before the change" % pbc, reset=True)
            b.lattice[1] *= 1.5
            lat = (c.lattice[0], float(b.lattice[1].item()), c.lattice[2])
            assert lat[1] == 1.5 * c.lattice[1] and R.pair_grid_ref(lat, c.sigma, R.XCUT, 800) == (19, 5, 2, 2, 13, 1)
            ref = R.pair_sum_ref(c.x, c.y, c.z, lat, pbc, c.sigma, R.K, q, R.XCUT)
            assert ref.margin >= 1e-9
            if pbc:
                assert int(ref.n_in.sum()) != int(R.reference("rect", pbc).n_in.sum())
            _step(hip, b, c._replace(lattice=lat), pbc, ref, 1, "rect pbc %d, ly x 1.5 in place" % pbc, reset=False)
        finally:
            _restore(L)


def test_positions_rewritten_in_place(hip):
    """The contract of the raw-pointer entry: positions rewritten behind the same pointers need dkmc_reset_pair_sum_cache(); after it the sums are
    those of the new positions (here rect's sites mirrored in y and z and reversed in order, so that every site changes its column)."""
    import torch
    host, L = hip
    c = R.case("rect")
    q = c.steps[0].q
    b = Box(c, q)
    try:
        _step(hip, b, c, 0, R.reference("rect", 0), 1, "rect before the rewrite", reset=True)
        lx, ly, lz = c.lattice
        x2, y2, z2 = c.x[::-1].copy(), (ly - c.y)[::-1].copy(), (lz - c.z)[::-1].copy()
        ptrs = (b.x.data_ptr(), b.y.data_ptr(), b.z.data_ptr())
        b.x.copy_(torch.as_tensor(x2)); b.y.copy_(torch.as_tensor(y2)); b.z.copy_(torch.as_tensor(z2))
        assert ptrs == (b.x.data_ptr(), b.y.data_ptr(), b.z.data_ptr())
        c2 = c._replace(x=x2, y=y2, z=z2)
        ref = R.pair_sum_ref(x2, y2, z2, c.lattice, 0, c.sigma, R.K, q, R.XCUT)
        assert ref.margin >= 1e-9 and ref.d2_min >= 1e-6
        _step(hip, b, c2, 0, ref, 1, "rect rewritten in place, cache reset", reset=True)
    finally:
        _restore(L)
