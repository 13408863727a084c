"""The cluster tracking on the device (dkmc_track_clusters, csrc/track.hip) against the host reference track_ref.py: the change codes, every column
of the three tables, the critical sites and info -- the x range included -- with np.array_equal."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_ref as cr
import track_ref as tr
from analysis_support import _dev, hip  # noqa: F401
from conftest import params_7p5
from track_ref import PINNED_2P5, PLANTINGS, check_pinned_2p5, random_pair

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 7, 63, 64, 65, 255, 256, 257, 1000, 5000)


@pytest.fixture(autouse=True)
def _default_hash(hip):
    yield
    hip[1].dkmc_debug_set_track_hash(0)


def run_raw(hip, label_prev, label_now, x, n_left, n_right):
    """the raw entry point on host arrays -> (site_change: host array, pairs, now, prev, critical, info)"""
    host, _ = hip
    res = host.track_clusters(_dev(label_prev, np.int32), _dev(label_now, np.int32), None if x is None else _dev(x, np.float64), n_left, n_right)
    return (res[0].cpu().numpy(),) + res[1:]


def check_raw(hip, label_prev, label_now, x, n_left, n_right, ref=None):
    ref = tr.analyse(label_prev, label_now, x, n_left, n_right) if ref is None else ref
    got = run_raw(hip, label_prev, label_now, x, n_left, n_right)
    tr.assert_equal(*got, ref)
    return got, ref


def _bytes(res):
    change, pairs, now, prev, critical, info = res
    return (change.tobytes() + b"".join(t[k].tobytes() for t, names in ((pairs, tr.PAIRS), (now, tr.NOW), (prev, tr.PREV)) for k in names)
            + critical.tobytes() + repr([info[k] for k in tr.INFO + ("critical_xmin", "critical_xmax")]).encode())


# ---- random label pairs: wave and workgroup edges, several workgroups -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_cases(N):
    """[(label_prev, label_now, x or None, n_left, n_right, reference)] with {1, 2, 5, N} ids per side; computed once, shared, never written to"""
    rng = np.random.default_rng(4000 + N)
    cases = []
    for k_prev in (1, 2, 5, N):
        for k_now in (1, 2, 5, N):
            lp, ln, x = random_pair(rng, N, k_prev, k_now, 0.8 if (k_prev + k_now) % 2 else 0.4)
            x = None if (k_prev, k_now) == (2, 5) else x
            nl, nr = (2, 3) if len(cases) % 2 else ((N + 3) // 4, (N + 2) // 3)      # thin contacts: open states among many random ids
            cases.append((lp, ln, x, nl, nr, tr.analyse(lp, ln, x, nl, nr)))
    return cases


@pytest.mark.parametrize("N", SIZES)
def test_random_pairs(hip, N):
    transitions = set()
    for lp, ln, x, nl, nr, ref in _random_cases(N):
        got, _ = check_raw(hip, lp, ln, x, nl, nr, ref)
        transitions.add(got[5]["transition"])
        if x is None:
            assert got[5]["critical_xmin"] == np.inf and got[5]["critical_xmax"] == -np.inf
    assert N < 63 or len(transitions) >= 3


@pytest.mark.parametrize("N", [n for n in SIZES if n <= 1000])
def test_longest_probe_chains_same_bytes(hip, N):
    """every key starts probing at the last slot: the chains grow as long as the table is full and wrap around; the bytes are those of the rule"""
    _, L = hip
    for lp, ln, x, nl, nr, ref in _random_cases(N):
        L.dkmc_debug_set_track_hash(0)
        plain = run_raw(hip, lp, ln, x, nl, nr)
        L.dkmc_debug_set_track_hash(1)
        chained = run_raw(hip, lp, ln, x, nl, nr)
        tr.assert_equal(*chained, ref)
        assert _bytes(plain) == _bytes(chained)


# ---- the shapes of the pair table ----------------------------------------------------------------------------------------------------------------
def test_all_sites_on_one_pair(hip):
    """the wave-combined path: every wave carries one pair, one counter takes them all"""
    N = 5000
    x = np.arange(N) * 0.25
    got, _ = check_raw(hip, np.full(N, 3, dtype=np.int32), np.full(N, 7, dtype=np.int32), x, 10, 10)
    change, pairs, now, prev, critical, info = got
    assert [pairs[k].tolist() for k in tr.PAIRS] == [[3], [7], [N], [0]] and (change == tr.STAYED).all()
    assert (info["transition"], info["bridge_prev"], info["bridge_now"], info["stayed"]) == (tr.BRIDGED, 3, 7, N)
    # two pairs that alternate lane by lane, and runs that end inside a wave
    lab = (np.arange(N) % 2).astype(np.int32)
    check_raw(hip, lab, lab[::-1].copy(), x, 10, 10)
    runs = (np.arange(N) // 37).astype(np.int32)
    check_raw(hip, runs, (np.arange(N) // 53).astype(np.int32), x, 10, 10)


@pytest.mark.parametrize("mode", [0, 1])
def test_all_pairs_distinct(hip, mode):
    """prev = arange, now = a permutation: N pairs, the fullest table the capacity rule allows"""
    _, L = hip
    N = 5000 if mode == 0 else 1000
    L.dkmc_debug_set_track_hash(mode)
    now = np.random.default_rng(8).permutation(N).astype(np.int32)
    got, _ = check_raw(hip, np.arange(N, dtype=np.int32), now, np.linspace(-1.0, 1.0, N), N // 10, N // 10)
    info = got[5]
    assert (info["n_pairs"], info["n_prev"], info["n_now"], info["stayed"], info["regrouped"], info["merged"], info["split"]) == (N, N, N, N, 0, 0, 0)
    assert np.array_equal(got[1]["first_site"], np.arange(N)) and np.array_equal(got[1]["now"], now)


def test_same_pointer_for_both_sides(hip):
    host, _ = hip
    lp, _, x, nl, nr, _ = _random_cases(1000)[10]
    t = _dev(lp, np.int32)
    res = host.track_clusters(t, t, _dev(x, np.float64), nl, nr)
    tr.assert_equal(res[0].cpu().numpy(), *res[1:], tr.analyse(lp, lp, x, nl, nr))
    info = res[5]
    assert info["joined"] == info["left"] == info["regrouped"] == info["born"] == info["died"] == 0 and info["transition"] in (tr.OPEN, tr.BRIDGED)
    assert np.array_equal(t.cpu().numpy(), lp)


def test_only_joiners_only_leavers_no_member_n_zero(hip):
    import torch
    host, _ = hip
    N = 700
    lab = random_pair(np.random.default_rng(3), N, 5, 5)[1]
    none = np.full(N, -1, dtype=np.int32)
    x = np.arange(N) * 1.5
    members = int((tr.sides(lab, N) >= 0).sum())
    got, _ = check_raw(hip, none, lab, x, 200, 200)
    assert got[5]["joined"] == members > 0 and got[5]["born"] == got[5]["n_now"] > 0 and got[5]["n_prev"] == 0 and len(got[3]["root"]) == 0
    got, _ = check_raw(hip, lab, none, x, 200, 200)
    assert got[5]["left"] == members and got[5]["died"] == got[5]["n_prev"] > 0 and got[5]["n_now"] == 0 and len(got[2]["root"]) == 0
    empty = dict(zip(tr.INFO, (0, 0, 0, 0, 0, 0, 0, 0, -1, -1, 0, 0, 0, 0, 0)), critical_xmin=np.inf, critical_xmax=-np.inf)
    got, _ = check_raw(hip, none, np.full(N, N, dtype=np.int32), x, 200, 200)
    assert got[5] == empty and not got[0].any() and len(got[1]["prev"]) == len(got[4]) == 0
    e = torch.empty(0, dtype=torch.int32, device="cuda:0")
    change, pairs, now, prev, critical, info = host.track_clusters(e, e, torch.empty(0, dtype=torch.float64, device="cuda:0"), 3, 3)
    assert info == empty and change.numel() == len(pairs["count"]) == len(now["root"]) == len(prev["root"]) == len(critical) == 0
    tr.assert_equal(change.cpu().numpy(), pairs, now, prev, critical, info, tr.analyse(np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), None, 3, 3))


def test_contact_clamping(hip):
    lp, ln, x, _, _, _ = _random_cases(257)[9]
    N = len(lp)
    for nl, nr in ((0, 0), (-4, 3 * N), (N, N)):
        got, _ = check_raw(hip, lp, ln, x, nl, nr)
        if (nl, nr) == (0, 0):
            assert got[5]["transition"] == tr.OPEN and not (got[2]["flags"] & 3).any() and not (got[3]["flags"] & 3).any()
        if (nl, nr) == (-4, 3 * N):
            assert ((got[2]["flags"] & 3) == tr.TOUCH_RIGHT).all() and ((got[3]["flags"] & 3) == tr.TOUCH_RIGHT).all()
        if (nl, nr) == (N, N):
            assert got[5]["transition"] == tr.BRIDGED and ((got[2]["flags"] & 3) == 3).all()


# ---- arguments and getters ------------------------------------------------------------------------------------------------------------------------
def test_getters_null_columns_and_capacity(hip):
    _, L = hip
    tips = np.array([0, 0, -1, -1, 4, 4, 6, -1], dtype=np.int32)
    full = np.array([0, 0, 0, 0, 0, 0, -1, 7], dtype=np.int32)
    got, _ = check_raw(hip, tips, full, np.arange(8) * 0.5, 1, 3)
    change, pairs, now, prev, critical, info = got
    assert (info["n_pairs"], info["n_now"], info["n_prev"], info["n_critical"], info["transition"]) == (5, 2, 3, 2, tr.CLOSED)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rows = C.c_int(-1)
    for call, table, names in ((L.dkmc_copy_track_pairs, pairs, tr.PAIRS), (L.dkmc_copy_track_now, now, tr.NOW), (L.dkmc_copy_track_prev, prev, tr.PREV),
                               (L.dkmc_copy_track_critical, dict(site=critical), ("site",))):
        n, k = len(table[names[0]]), len(names)
        assert call(10 ** 6, *([None] * k), C.byref(rows)) == 0 and rows.value == n
        assert call(10 ** 6, *([None] * k), None) == 0
        assert call(0, *([None] * k), C.byref(rows)) == 0 and rows.value == 0
        assert call(-3, *([None] * k), C.byref(rows)) == 0 and rows.value == 0
        for j in range(k):                                                         # one column at a time, the others NULL, one row short
            col = np.full(n + 2, -9, dtype=np.int32)
            args = [None] * k
            args[j] = vp(col)
            assert call(n - 1, *args, C.byref(rows)) == 0 and rows.value == n - 1
            assert np.array_equal(col[:n - 1], table[names[j]][:n - 1]) and (col[n - 1:] == -9).all()
        cols = [np.full(n + 2, -9, dtype=np.int32) for _ in names]
        assert call(n + 2, *[vp(c) for c in cols], C.byref(rows)) == 0 and rows.value == n
        assert all(np.array_equal(c[:n], table[m]) and (c[n:] == -9).all() for c, m in zip(cols, names))
    i16, x2 = (C.c_longlong * 16)(), (C.c_double * 2)()
    assert L.dkmc_get_track_info(None, None) == 0 and L.dkmc_get_track_info(i16, None) == 0 and L.dkmc_get_track_info(None, x2) == 0
    assert list(i16) == [info[k] for k in tr.INFO] + [0] and list(x2) == [1.0, 1.5] == [info["critical_xmin"], info["critical_xmax"]]


def test_bad_arguments(hip):
    import torch
    host, L = hip
    n = 100
    lab = _dev(np.zeros(n), np.int32)
    change = torch.full((n,), 7, dtype=torch.int32, device="cuda:0")
    pl, pc = host._ptr(lab), host._ptr(change)
    assert L.dkmc_track_clusters(n, pl, pl, None, 1, 1, pc) == 0 and L.dkmc_get_track_info(None, None) == 0
    rows = C.c_int(0)
    for args in ((-1, pl, pl, None, 1, 1, pc), (n, None, pl, None, 1, 1, pc), (n, pl, None, None, 1, 1, pc), (n, pl, pl, None, 1, 1, None)):
        change.fill_(7)
        assert L.dkmc_track_clusters(*args) == 3
        assert "dkmc_track_clusters" in L.dkmc_last_error().decode()
        L.dkmc_clear_error()
        for call in (lambda: L.dkmc_get_track_info(None, None), lambda: L.dkmc_copy_track_pairs(4, None, None, None, None, C.byref(rows)),
                     lambda: L.dkmc_copy_track_now(4, None, None, None, None, None, None, C.byref(rows)),
                     lambda: L.dkmc_copy_track_prev(4, None, None, None, None, None, None, C.byref(rows)),
                     lambda: L.dkmc_copy_track_critical(4, None, C.byref(rows)), lambda: L.dkmc_debug_get_track_times(None)):
            assert call() == 3                                                     # no results of a failed call
            L.dkmc_clear_error()
        torch.cuda.synchronize()
        assert (change.cpu().numpy() == 7).all()                                   # nothing was launched
    assert L.dkmc_track_clusters(0, None, None, None, 1, 1, None) == 0 and L.dkmc_get_track_info(None, None) == 0


_FRESH = """
import ctypes as C, sys
sys.path.insert(0, %r)
from devicekmc_amd import lib
L = lib.load()
rows = C.c_int(0)
def getters():
    out = [L.dkmc_get_track_info(None, None), L.dkmc_copy_track_pairs(4, None, None, None, None, C.byref(rows)),
           L.dkmc_copy_track_now(4, None, None, None, None, None, None, C.byref(rows)),
           L.dkmc_copy_track_prev(4, None, None, None, None, None, None, C.byref(rows)),
           L.dkmc_copy_track_critical(4, None, C.byref(rows)), L.dkmc_debug_get_track_times(None)]
    msg = L.dkmc_last_error().decode()
    L.dkmc_clear_error()
    return out, msg
before, msg = getters()
bad = L.dkmc_track_clusters(-1, None, None, None, 0, 0, None)
L.dkmc_clear_error()
between, _ = getters()
ok = L.dkmc_track_clusters(0, None, None, None, 0, 0, None)
after, _ = getters()
print(before, "dkmc_debug_get_track_times" in msg, bad, between, ok, after)
"""


def test_getters_fail_before_the_first_success(hip):
    """in a fresh process: another test of this module may have succeeded first in this one"""
    out = subprocess.run([sys.executable, "-c", _FRESH % ROOT], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "%s True 3 %s 0 %s" % ([3] * 6, [3] * 6, [0] * 6)


# ---- repeatability -----------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_same_bytes(hip):
    lp, ln, x, nl, nr, ref = _random_cases(5000)[15]
    a = run_raw(hip, lp, ln, x, nl, nr)
    b = run_raw(hip, lp, ln, x, nl, nr)
    tr.assert_equal(*a, ref)
    assert a[5]["n_pairs"] > 1000 and _bytes(a) == _bytes(b)


# ---- the golden devices ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev_2p5(hip, cell_2p5):
    from devicekmc_amd import params as pm
    host, _ = hip
    p = pm.KMCParameters()
    dev = host.Device(cell_2p5, p)
    return dev, dev.make_gpubuf("cuda:0"), p, dev.site_element.copy()


def _set_elements(dev, gb, el):
    import torch
    dev.site_element = el.copy()
    gb.t["site_element"].copy_(torch.as_tensor(el))


def _planted(dev, el0, name):
    return el0 if PLANTINGS[name] is None else cr.plant_filament(el0, dev.site_x, dev.site_y, dev.site_z, *PLANTINGS[name])[0]


@pytest.mark.parametrize("key", list(PINNED_2P5), ids=["-".join(k) for k in PINNED_2P5])
def test_pinned_transitions_2p5(hip, dev_2p5, key):
    """Device.find_clusters twice + Device.track_clusters on the real buffers, the planting through gpubuf.site_element"""
    dev, gb, p, el0 = dev_2p5
    try:
        labels = []
        for name in key:
            _set_elements(dev, gb, _planted(dev, el0, name))
            labels.append(dev.find_clusters(gb)[0])
        nl, nr = dev.contact_seeds()
        res = dev.track_clusters(gb)
        print(key, res[5])
        tr.assert_equal(*res, tr.analyse(labels[0], labels[1], dev.site_x, nl, nr))
        check_pinned_2p5(key, res)
        assert dev.site_change is res[0] and dev.track_pairs is res[1] and dev.track_now is res[2] and dev.track_prev is res[3]
        assert dev.track_critical is res[4] and dev.track_info is res[5]
        assert np.array_equal(dev._cluster_label_prev.cpu().numpy(), labels[0]) and np.array_equal(dev._cluster_label.cpu().numpy(), labels[1])
        # given labels replace the kept ones: the same transition backwards
        back = dev.track_clusters(gb, label_prev=dev._cluster_label, label_now=dev._cluster_label_prev)
        tr.assert_equal(*back, tr.analyse(labels[1], labels[0], dev.site_x, nl, nr))
        assert back[5]["joined"] == res[5]["left"] and back[5]["n_critical"] == res[5]["n_critical"]
    finally:
        _set_elements(dev, gb, el0)


def test_fewer_than_two_analyses_raise(hip, dev_2p5, cell_2p5):
    host, _ = hip
    _, gb, p, _ = dev_2p5
    dev = host.Device(cell_2p5, p)
    with pytest.raises(ValueError, match="fewer than two"):
        dev.track_clusters(gb)
    dev.find_clusters(gb)
    with pytest.raises(ValueError, match="fewer than two"):
        dev.track_clusters(gb)
    dev.find_clusters(gb)
    assert dev.track_clusters(gb)[5]["transition"] == tr.OPEN and dev.track_info["n_pairs"] == 79


def test_open_to_full_7p5(hip, dev_7p5):
    host, _ = hip
    p = params_7p5()
    dev = host.Device(dev_7p5, p, gpu_neighbors="cuda:0")
    gb = dev.make_gpubuf("cuda:0")
    el0 = dev.site_element.copy()
    labels = []
    for name in ("open", "full"):
        _set_elements(dev, gb, _planted(dev, el0, name))
        labels.append(dev.find_clusters(gb)[0])
    res = dev.track_clusters(gb)
    nl, nr = dev.contact_seeds()
    tr.assert_equal(*res, tr.analyse(labels[0], labels[1], dev.site_x, nl, nr))
    info = res[5]
    assert info["transition"] == tr.CLOSED and info["n_critical"] == info["joined"] > 0 and info["left"] == 0


def test_three_current_off_supersteps_2p5(hip, cell_2p5):
    """find_clusters after every superstep, tracking between consecutive ones, against the reference on the downloaded labels"""
    from devicekmc_amd import params as pm
    host, _ = hip
    p = pm.KMCParameters()
    dev = host.Device(cell_2p5, p); sim = host.KMCProcess(dev, p.freq); gb = dev.make_gpubuf("cuda:0")
    dev.setLaplacePotential(gb, p, 5.0); gb.sync_HostToGPU(dev)
    nl, nr = dev.contact_seeds()
    labels = [dev.find_clusters(gb)[0]]
    moved = 0
    for step in range(3):
        dev.updateCharge(gb)
        dev.updatePotential(gb, p, 5.0, step)
        sim.executeKMCStep(gb, dev)
        labels.append(dev.find_clusters(gb)[0])
        members = dev.cluster_info["n_members"]
        res = dev.track_clusters(gb)
        tr.assert_equal(*res, tr.analyse(labels[-2], labels[-1], dev.site_x, nl, nr))
        info = res[5]
        assert info["stayed"] + info["joined"] == members and info["n_now"] == dev.cluster_info["n_components"]
        moved += info["joined"] + info["left"]
    print("sites that joined or left over the three steps:", moved)
