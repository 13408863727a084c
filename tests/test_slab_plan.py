"""The integer bookkeeping of the slab partition (csrc/slab_plan.h), on the CPU: tests/cpu/slab_plan_check.cpp includes that header alone, is
compiled with -fsanitize=address,undefined and run as a plain program.  It allocates every list and exchange buffer at EXACTLY the plan's total and
fills it through the plan's offsets, so an offset that is off ends in a sanitizer report, a gap or a wrong order.  The rules, restated here:
  rowoff / markoff  running sums of the rows / marked rows per owner; maxown the largest slab; covers: both totals as expected;
  halo lists of v   pieces in rank order, v itself left out: to d hal[v][d] rows, from s hal[s][v] rows;
  all-to-all-v      cnt[a][d] doubles a -> d: in a's send buffer the pieces lie in destination order, in d's receive buffer in source order; a rank
                    sends its row sum and receives its column sum; recvmax = the largest column sum without its diagonal entry."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("slab_plan") / "slab_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "devicekmc_amd", "csrc"), os.path.join(ROOT, "tests", "cpu", "slab_plan_check.cpp"), "-o", exe], check=True)

    def run(*args):
        r = subprocess.run([exe] + [str(int(a)) if not isinstance(a, str) else a for a in args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (args[:3], r.stdout[-2000:], r.stderr[-4000:])
        assert r.stderr == "", r.stderr[-4000:]                  # a sanitizer report goes here
        out = {}
        for line in r.stdout.splitlines():
            f = line.split()
            out[f[0]] = [int(x) for x in f[1:]]
        return out
    return run


def _table(nown, nmark, hal):
    return list(nown) + list(nmark) + [int(x) for x in np.asarray(hal).reshape(-1)]


def _hal(nr, rule):
    return np.array([[0 if s == d else rule(s, d) for d in range(nr)] for s in range(nr)], dtype=np.int64).reshape(nr, nr)


rng = np.random.RandomState(7)
PLANS = {
    "nr1": ([12], [5], _hal(1, lambda s, d: 0)),
    "nr2": ([7, 5], [0, 3], _hal(2, lambda s, d: 2 + s)),
    "nr3": ([4, 4, 4], [1, 2, 3], _hal(3, lambda s, d: 1 + 3 * s + d)),
    "empty_front": ([0, 6, 6], [0, 2, 1], _hal(3, lambda s, d: 0 if 0 in (s, d) else 2)),
    "empty_middle": ([3, 6, 0, 1], [3, 0, 0, 1], _hal(4, lambda s, d: 0 if 2 in (s, d) else 1 + d)),
    "empty_end": ([5, 5, 0], [1, 1, 0], _hal(3, lambda s, d: 0 if 2 in (s, d) else 3)),
    "no_halo": ([9, 9, 9], [0, 0, 0], _hal(3, lambda s, d: 0)),
    "nr32": (list(rng.randint(0, 50, 32)), list(rng.randint(0, 9, 32)), _hal(32, lambda s, d: int(rng.randint(0, 4)) if abs(s - d) < 3 else 0)),
}


@pytest.mark.parametrize("name", sorted(PLANS))
def test_offsets_by_owner_and_halo_lists(check, name):
    nown, nmark, hal = PLANS[name]
    nr = len(nown)
    out = check("plan", nr, sum(nown), sum(nmark), *_table(nown, nmark, hal))
    assert out["rowoff"] == [0] + list(np.cumsum(nown)) and out["markoff"] == [0] + list(np.cumsum(nmark))
    assert out["maxown"] == [max(nown)] and out["covers"] == [1]
    for v in range(nr):
        to = [0 if d == v else int(hal[v, d]) for d in range(nr)]
        frm = [0 if s == v else int(hal[s, v]) for s in range(nr)]
        assert out["hsoff%d" % v] == [0] + list(np.cumsum(to)) and out["hroff%d" % v] == [0] + list(np.cumsum(frm)), v
        # the pieces tile the lists without gap or overlap, in rank order
        assert out["hsend%d" % v] == [d for d in range(nr) for _ in range(to[d])], v
        assert out["hrecv%d" % v] == [s for s in range(nr) for _ in range(frm[s])], v
    # the cover test answers no when a row or a marked row is missing
    assert check("plan", nr, sum(nown) + 1, sum(nmark), *_table(nown, nmark, hal))["covers"] == [0]
    assert check("plan", nr, sum(nown), sum(nmark) + 1, *_table(nown, nmark, hal))["covers"] == [0]


def _one(nr, a, d, n):
    c = np.zeros((nr, nr), dtype=np.int64); c[a, d] = n
    return c


A2A = {
    "nr1_self": np.array([[5]]),
    "nr1_zero": np.array([[0]]),
    "nr2": np.array([[0, 3], [4, 0]]),
    "nr3_all_zero": np.zeros((3, 3), dtype=np.int64),
    "nr3_one_piece": _one(3, 2, 0, 7),
    "nr3_one_piece_diag": _one(3, 1, 1, 4),
    "nr3_all_equal": np.full((3, 3), 5),
    "nr3_with_diag": np.array([[9, 1, 2], [3, 9, 4], [5, 6, 9]]),             # exchange 1 of the X loop keeps a piece for the rank itself
    "nr3_empty_rank": np.array([[0, 0, 2], [0, 0, 0], [3, 0, 0]]),
    "nr32_all_equal": np.full((32, 32), 3),
    "nr32_one_piece": _one(32, 31, 0, 2),
    "nr32_random": np.random.RandomState(3).randint(0, 6, (32, 32)) * (np.random.RandomState(4).rand(32, 32) < 0.3),
}


@pytest.mark.parametrize("name", sorted(A2A))
def test_all_to_all_v_pieces_tile_both_buffers(check, name):
    cnt = np.asarray(A2A[name], dtype=np.int64)
    nr = cnt.shape[0]
    out = check("a2a", nr, *cnt.reshape(-1))
    for r in range(nr):
        # send pieces in destination order, receive pieces in source order, no gap (-1) and no overlap; totals = row and column sums
        assert out["send%d" % r] == [d for d in range(nr) for _ in range(cnt[r, d])], r
        assert out["recv%d" % r] == [a for a in range(nr) for _ in range(cnt[a, r])], r
        assert len(out["send%d" % r]) == cnt[r].sum() and len(out["recv%d" % r]) == cnt[:, r].sum()
    assert out["recvmax"] == [max(int(cnt[:, d].sum() - cnt[d, d]) for d in range(nr))]


def test_reference_partitions_of_the_gpu_cases():
    """tests/slab_ref.py (the reference of tests/test_gpu_slab_plan.py) on its own cases: what the rule gives where it can be worked out by hand."""
    import slab_ref
    C = slab_ref.cases()
    part = {n: slab_ref.partition(c["m"], c["first"], c["rp"], c["ci"], c["coord"], c["lo"], c["hi"], c["nr"], c["mark"]) for n, c in C.items() if c["m"] < 1000}
    a = part["a_chain_one_rank"]
    assert list(a["nown"]) == [12] and not a["mask"].any() and not a["hal"].any()
    b = part["b_ring_three_ranks"]
    assert list(b["nown"]) == [4, 4, 4] and np.array_equal(b["hal"], 1 - np.eye(3, dtype=np.int64))         # one halo row for every ordered pair
    assert list(slab_ref.halo_lists(b, 0, 3, 0)[0]) == [3, 0] and list(slab_ref.halo_lists(b, 0, 3, 0)[1]) == [4, 11]
    c = part["c_driver_rows_and_marks"]
    assert list(c["nown"]) == [4, 4, 4] and list(c["nmark"]) == [2, 1, 1] and not c["mask"][:2].any() and list(c["owner"][:2]) == [0, 0]
    assert np.array_equal(c["hal"], [[0, 1, 0], [1, 0, 1], [0, 1, 0]]) and c["rows_by_owner"].min() == 2
    assert list(part["d_all_in_one_bin"]["nown"]) == [12, 0, 0]
    e = part["e_thirty_two_ranks"]
    assert e["owner"].max() == 31 and e["mask"][38] == 0xa0000000
    for k in ("owner", "mask", "tab", "rows_by_owner"):
        assert np.array_equal(part["f_class_bit_31"][k], b[k]), k
    assert list(part["g_heavy_bin_empty_slab"]["nown"]) == [3, 6, 0, 1]
    assert list(part["h_clamped_ends"]["nown"]) == [5, 5]


def test_table_buffer_layout(check):
    """hist[4096] | cuts[34] | tab[32 * 34]: the three parts tile the buffer of slab_tab_bytes() (every int written exactly once)."""
    out = check("layout")
    assert out["bytes"] == [(4096 + 34 + 32 * 34) * 4] and out["sum"] == [4096 * 1 + 34 * 2 + 32 * 34 * 3]
