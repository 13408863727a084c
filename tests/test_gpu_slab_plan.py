"""The slab partition both distributed loops share (csrc/slab.h: one partition step, rows_by_owner, the halo lists; csrc/slab_plan.h: their offsets)
at small shapes, through the test aid dkmc_debug_slab_plan, against the numpy restatement of the rule in tests/slab_ref.py.  Whole solves reach this
code only on the 85 071-site device, where a wrong list shows as "the virtual ranks disagree"; here owner, mask, the whole count table,
rows_by_owner and both halo lists of EVERY rank must equal the reference exactly.  The cases (slab_ref.cases): one rank; a ring over three ranks (a
halo to a non-adjacent slab); replicated driver rows and marked rows; every row in one bin (two empty slabs); 32 ranks (bit 31 of the masks); the
class bit 31 on column words; a heavy bin across two cuts (an empty slab in the middle); coordinates outside lo ... hi; and 140 000 rows -- above the
131 072 rows one pass of k_slab_count's grid covers and above one block of the scan."""
import ctypes as C

import numpy as np
import pytest

import slab_ref
from devicekmc_amd.lib import check
from test_gpu_parity import hip  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = slab_ref.cases()


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _run(L, c, v, lists=True):
    m, first, nr = c["m"], c["first"], c["nr"]
    rp, ci = np.ascontiguousarray(c["rp"], dtype=np.int32), np.ascontiguousarray(c["ci"], dtype=np.int32)
    coord = np.ascontiguousarray(c["coord"], dtype=np.float64)
    mark = None if c["mark"] is None else np.ascontiguousarray(c["mark"], dtype=np.int32)
    owner, mask = np.full(m, -7, dtype=np.int32), np.full(m, 0xdeadbeef, dtype=np.uint32)
    tab, rbo = np.full(nr * (nr + 2), -7, dtype=np.int32), np.full(m - first, -7, dtype=np.int32)
    # room for the longest list there can be: every distributed row to (from) every other rank
    hs, hr = np.full((m - first) * max(nr - 1, 1), -7, dtype=np.int32), np.full((m - first) * max(nr - 1, 1), -7, dtype=np.int32)
    check(L.dkmc_debug_slab_plan(m, first, _p(rp), _p(ci), _p(coord), c["lo"], c["hi"], nr, _p(mark), v, _p(owner), _p(mask), _p(tab), _p(rbo),
                                 _p(hs) if lists else None, _p(hr) if lists else None))
    return owner, mask, tab, rbo, hs, hr


@pytest.mark.parametrize("name", sorted(CASES))
def test_partition_and_lists_equal_the_reference(hip, name):
    _, L = hip
    c = CASES[name]
    m, first, nr = c["m"], c["first"], c["nr"]
    ref = slab_ref.partition(m, first, c["rp"], c["ci"], c["coord"], c["lo"], c["hi"], nr, c["mark"])
    sends, recvs = {}, {}
    for v in range(nr):
        owner, mask, tab, rbo, hs, hr = _run(L, c, v)
        assert np.array_equal(owner, ref["owner"]), (name, v)
        assert np.array_equal(mask, ref["mask"]), (name, v)
        assert np.array_equal(tab, ref["tab"]), (name, v, tab, ref["tab"])
        assert np.array_equal(rbo, ref["rows_by_owner"]), (name, v)
        assert np.array_equal(np.sort(rbo), np.arange(first, m)), (name, v)                       # a permutation of the distributed rows
        rs, rr = slab_ref.halo_lists(ref, first, nr, v)
        assert np.array_equal(hs[:len(rs)], rs) and np.all(hs[len(rs):] == -7), (name, v, hs[:len(rs) + 4], rs)
        assert np.array_equal(hr[:len(rr)], rr) and np.all(hr[len(rr):] == -7), (name, v, hr[:len(rr) + 4], rr)
        # the pieces by peer, at the offsets the table implies
        hal = tab[2 * nr:].reshape(nr, nr)
        so = np.concatenate(([0], np.cumsum([0 if d == v else hal[v, d] for d in range(nr)])))
        ro = np.concatenate(([0], np.cumsum([0 if s == v else hal[s, v] for s in range(nr)])))
        for d in range(nr):
            sends[(v, d)] = hs[so[d]:so[d + 1]].copy()
            recvs[(d, v)] = hr[ro[d]:ro[d + 1]].copy()
    for s in range(nr):
        for d in range(nr):
            assert np.array_equal(sends[(s, d)], recvs[(s, d)]), (name, s, d)                     # what s sends to d is what d receives from s
            assert np.all(np.diff(sends[(s, d)]) > 0), (name, s, d)                               # ascending


def test_table_only_call_and_bad_arguments(hip):
    """hsend / hrecv null: the per-row outputs and the table all the same; a column outside the pattern, a rank outside 1 ... 32 and a v outside the
    ranks are refused before anything is launched."""
    _, L = hip
    c = CASES["b_ring_three_ranks"]
    ref = slab_ref.partition(c["m"], c["first"], c["rp"], c["ci"], c["coord"], c["lo"], c["hi"], c["nr"], c["mark"])
    owner, mask, tab, rbo, hs, hr = _run(L, c, 1, lists=False)
    assert np.array_equal(owner, ref["owner"]) and np.array_equal(mask, ref["mask"]) and np.array_equal(tab, ref["tab"]) and np.array_equal(rbo, ref["rows_by_owner"])
    assert np.all(hs == -7) and np.all(hr == -7)
    bad = dict(c, ci=c["ci"].copy()); bad["ci"][3] = c["m"]
    from devicekmc_amd.lib import DeviceKMCError
    for cc, v in ((bad, 0), (dict(c, nr=33), 0), (c, 3), (c, -1)):
        with pytest.raises(DeviceKMCError, match="debug_slab_plan"):
            _run(L, cc, v)
