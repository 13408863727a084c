"""The cut-site analysis on the device (dkmc_find_cuts, csrc/cuts.hip) against the host reference cut_ref.py: both site arrays, every column of
the three tables -- doubles included -- and info with np.array_equal; the number of labelling rounds against the reference's synchronous model."""
import ctypes as C

import numpy as np
import pytest

import cluster_ref as cr
import cut_ref as cu
import path_ref as pr
from analysis_support import SHAPES, _chain, _dev, _random_case, hip, index_of, ladder  # noqa: F401
from conftest import params_7p5
from cut_ref import PINNED_2P5, PINNED_2P5_WIDE_BYPASS

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _default_cap(hip):
    yield
    hip[1].dkmc_debug_set_cut_round_cap(0)


def run_raw(hip, index, label, x, n_left, n_right, path):
    """the raw entry point on host arrays -> (site_role, site_bypass: host arrays, path table, bypasses, necks, info)"""
    host, _ = hip
    index = np.asarray(index)
    role, bypass, table, byp, necks, info = host.find_cuts(_dev(index, np.int32), index.shape[1], _dev(label, np.int32),
                                                           None if x is None else _dev(x, np.float64), n_left, n_right, path)
    return role.cpu().numpy(), bypass.cpu().numpy(), table, byp, necks, info


def check_raw(hip, index, label, x, n_left, n_right, path):
    ref = cu.analyse(index, label, x, n_left, n_right, path)
    got = run_raw(hip, index, label, x, n_left, n_right, path)
    cu.assert_equal(*got, ref)
    return got


def _bytes(res):
    role, bypass, table, byp, necks, info = res
    cols = [table[k] for k in cu.PATH] + [byp[k] for k in cu.BYPASSES] + [necks[k] for k in cu.NECKS]
    return role.tobytes() + bypass.tobytes() + b"".join(c.tobytes() for c in cols) + repr([info[k] for k in cu.INFO]).encode()


# ---- random graphs: workgroup and wave edges, every row-lane template, the whole-wave row ---------------------------------------------------
@pytest.mark.parametrize("one_way", [False, True])
@pytest.mark.parametrize("N,nn,p_member,p_pad", SHAPES)
def test_random_graphs(hip, N, nn, p_member, p_pad, one_way):
    rng = np.random.default_rng(1000 * N + nn + one_way)
    nl = nr = max(1, (2 * N) // 5)
    connected = 0
    for trial in range(2):
        index, element, _, x = _random_case(rng, N, nn, p_member, p_pad, one_way)
        index[rng.random(N) < 0.1] = -1                                             # padding-only rows
        index[rng.random((N, nn)) < 0.02] = N + 3                                   # padding past the end
        # labels outside 0 ... N - 1 are non-members, whatever their value
        label = np.where(element != 3, rng.integers(0, N, N), rng.choice([-1, N, N + 7, 2 ** 31 - 1, -2 ** 31], N)).astype(np.int32)
        check_raw(hip, index, label, x, nl, nr, [])                                 # status 0: the off-path components are all components
        canon = pr.analyse(index, label, x, nl, nr, 0)[2]
        if len(canon) == 0:
            continue
        connected += 1
        check_raw(hip, index, label, x, nl, nr, canon)
        _, ptr, nb, sl, sr = cu.graph(index, label, nl, nr)
        check_raw(hip, index, label, None, nl, nr, cu.random_simple_path(rng, ptr, nb, sl, sr))
    assert connected > 0


# ---- chains and ladders -------------------------------------------------------------------------------------------------------------------
def test_ordered_chain(hip):
    n = 300
    x = np.arange(n) * 0.5
    role, bypass, table, byp, necks, info = check_raw(hip, _chain(np.arange(n)), np.zeros(n, dtype=np.int32), x, 1, 1, np.arange(n))
    assert [info[k] for k in cu.INFO] == [1, n, n, 1, n, 0, 0, 0, 0, 0, 0, 1] and (role == cu.CUT).all() and (bypass == -1).all()
    assert (necks["first"].tolist(), necks["last"].tolist(), necks["xmin"].tolist(), necks["xmax"].tolist()) == ([0], [n - 1], [0.0], [x[-1]])


def test_randomly_numbered_chain(hip):
    """a path longer than any LDS-resident table, over sites in random order"""
    n = 2000
    order = np.r_[0, 1 + np.random.default_rng(11).permutation(n - 2), n - 1]
    got = check_raw(hip, _chain(order), np.zeros(n, dtype=np.int32), np.linspace(0.0, 1.0, n), 1, 1, order)
    assert got[5]["cut_sites"] == n and got[5]["necks"] == 1 and np.array_equal(got[2]["site"], order)


def test_ladder(hip):
    length = 500
    n = 2 * length
    index, label = index_of(ladder(length), n), np.zeros(n, dtype=np.int32)
    path = 2 * np.arange(length)
    role, bypass, table, byp, necks, info = check_raw(hip, index, label, np.arange(n) * 0.25, 2, 2, path)
    assert info["cut_sites"] == 0 and (table["n_bypass"] == 1).all() and (byp["lo"].tolist(), byp["hi"].tolist(), byp["size"].tolist()) == ([-1], [length], [length])
    # along the other rail, and along a path that changes rails at every rung but the last: the rails' links are chords then
    check_raw(hip, index, label, None, 2, 2, path + 1)
    zig = np.arange(n)
    zig[2::4], zig[3::4] = np.arange(n)[3::4], np.arange(n)[2::4]
    got = check_raw(hip, index, label, None, 2, 2, zig[:-1])
    assert got[5]["chord_positions"] > 0 and got[5]["cut_sites"] == 0


def _chain_with_side_branches(n_path, n_side, seed):
    """an ordered chain of n_path sites (the path), a randomly numbered chain of n_side sites hanging on position 10 (a side component, many
    labelling rounds) and a second one linking positions 20 and 60 (a bypass)"""
    rng = np.random.default_rng(seed)
    n = n_path + 2 * n_side
    a = n_path - 1 + rng.permutation(n_side)                                        # the last path site keeps the largest index
    b = n_path - 1 + n_side + rng.permutation(n_side)
    links = [(i, i + 1) for i in range(n_path - 2)] + [(n_path - 2, n - 1)]
    links += [(10, a[0])] + list(zip(a[:-1], a[1:])) + [(20, b[0])] + list(zip(b[:-1], b[1:])) + [(b[-1], 60)]
    return index_of(links, n, 3), np.r_[np.arange(n_path - 1), n - 1]


def test_side_branches_take_many_rounds(hip):
    index, path = _chain_with_side_branches(100, 3000, 4)
    n = len(index)
    got = check_raw(hip, index, np.zeros(n, dtype=np.int32), np.arange(n) * 1.0, 1, 1, path)
    role, bypass, table, byp, necks, info = got
    assert info["rounds"] > 8 and info["bypasses"] == 1 and (byp["lo"][0], byp["hi"][0], byp["size"][0]) == (20, 60, 3000)         # more than one batch
    assert info["offpath_components"] == 2 and info["cut_sites"] == 100 - 39 and info["necks"] == 2 and int((role == cu.SIDE).sum()) == 3000


def test_round_cap_fails_cleanly(hip):
    """an error return, not a device fault: the error is set, both site arrays are -1, the getters fail; the next call with the cap restored succeeds"""
    import torch
    host, L = hip
    idx, path = _chain_with_side_branches(100, 3000, 4)
    n = len(idx)
    index, label, dpath = _dev(idx, np.int32), _dev(np.zeros(n), np.int32), _dev(path, np.int32)
    role = torch.full((n,), 7, dtype=torch.int32, device="cuda:0")
    bypass = torch.full((n,), 7, dtype=torch.int32, device="cuda:0")
    L.dkmc_debug_set_cut_round_cap(3)
    rc = L.dkmc_find_cuts(n, 3, host._ptr(index), host._ptr(label), None, 1, 1, host._ptr(dpath), len(path), host._ptr(role), host._ptr(bypass))
    assert rc != 0 and "dkmc_find_cuts" in L.dkmc_last_error().decode() and "3 rounds" in L.dkmc_last_error().decode()
    L.dkmc_clear_error()
    torch.cuda.synchronize()
    assert (role.cpu().numpy() == -1).all() and (bypass.cpu().numpy() == -1).all()
    _getters_fail(L)
    L.dkmc_debug_set_cut_round_cap(0)
    got = check_raw(hip, idx, np.zeros(n, dtype=np.int32), None, 1, 1, path)
    assert got[5]["status"] == 1 and L.dkmc_get_cut_info(None) == 0


def _getters_fail(L):
    rows = C.c_int(0)
    for call in (lambda: L.dkmc_get_cut_info(None), lambda: L.dkmc_copy_cut_path(4, None, None, None, None, C.byref(rows)),
                 lambda: L.dkmc_copy_cut_bypasses(4, None, None, None, None, C.byref(rows)),
                 lambda: L.dkmc_copy_cut_necks(4, None, None, None, None, C.byref(rows)), lambda: L.dkmc_debug_get_cut_times(None)):
        assert call() == 3
        L.dkmc_clear_error()


# ---- status 0 -------------------------------------------------------------------------------------------------------------------------------
def test_status_zero(hip):
    import torch
    host, _ = hip
    rng = np.random.default_rng(5)
    N = 500
    index, element, _, x = _random_case(rng, N, 4, 0.7, 0.4, False)
    label = np.where(element != 3, 0, -1).astype(np.int32)
    role, bypass, table, byp, necks, info = check_raw(hip, index, label, x, 100, 100, [])
    assert info["status"] == 0 and info["offpath_members"] == int((label == 0).sum()) and (role[label == 0] == cu.APART).all()
    assert len(table["site"]) == len(byp["root"]) == len(necks["first"]) == 0
    assert np.array_equal(bypass, cr.labels_of(index, label == 0))                  # the canonical labels of the filament analysis
    # no member at all
    got = check_raw(hip, index, np.full(N, -1, dtype=np.int32), x, 100, 100, [])
    assert [got[5][k] for k in cu.INFO] == [0, 0, 0, 0, 0, -1, 0, 0, 0, 0, 0, 1] and (got[0] == 0).all() and (got[1] == -1).all()
    # N == 0
    e = torch.empty(0, dtype=torch.int32, device="cuda:0")
    role, bypass, table, byp, necks, info = host.find_cuts(e, 3, e, torch.empty(0, dtype=torch.float64, device="cuda:0"), 0, 0, None)
    assert [info[k] for k in cu.INFO] == [0, 0, 0, 0, 0, -1, 0, 0, 0, 0, 0, 0] and role.numel() == bypass.numel() == len(table["site"]) == 0


# ---- invalid paths --------------------------------------------------------------------------------------------------------------------------
_R12 = list(range(12))


@pytest.mark.parametrize("path,row,what", [([0, 1, 2, 3, 2, 3] + _R12[4:10], 4, "repeats"), (_R12[:3] + _R12[4:], 3, "not linked"),
                                           (_R12[1:], 0, "left seed"), (_R12[:11], 10, "right seed"),
                                           (_R12, 5, "not a member"), (_R12[:5] + [13] + _R12[6:], 5, "not a member"),
                                           (_R12[:5] + [-1] + _R12[6:], 5, "not a member")])
def test_invalid_paths(hip, path, row, what):
    """each one an error return with both arrays -1 and the getters failing, and the next valid call succeeds"""
    import torch
    host, L = hip
    n = 12
    idx = _chain(np.arange(n))
    lab = np.zeros(n, dtype=np.int32)
    if path == _R12:
        lab[5] = -1
    with pytest.raises(ValueError, match="row %d" % row):
        cu.analyse(idx, lab, None, 1, 1, path)
    index, label, dpath = _dev(idx, np.int32), _dev(lab, np.int32), _dev(path, np.int32)
    role = torch.full((n,), 7, dtype=torch.int32, device="cuda:0")
    bypass = torch.full((n,), 7, dtype=torch.int32, device="cuda:0")
    rc = L.dkmc_find_cuts(n, 2, host._ptr(index), host._ptr(label), None, 1, 1, host._ptr(dpath), len(path), host._ptr(role), host._ptr(bypass))
    msg = L.dkmc_last_error().decode()
    assert rc != 0 and "dkmc_find_cuts" in msg and "row %d " % row in msg and what in msg, msg
    L.dkmc_clear_error()
    torch.cuda.synchronize()
    assert (role.cpu().numpy() == -1).all() and (bypass.cpu().numpy() == -1).all()
    _getters_fail(L)
    got = check_raw(hip, idx, np.zeros(n, dtype=np.int32), None, 1, 1, np.arange(n))
    assert got[5]["cut_sites"] == n and L.dkmc_get_cut_info(None) == 0


# ---- arguments and getters ------------------------------------------------------------------------------------------------------------------
def test_bad_arguments(hip):
    import torch
    host, L = hip
    n = 100
    index, label, path = _dev(_chain(np.arange(n)), np.int32), _dev(np.zeros(n), np.int32), _dev(np.arange(n), np.int32)
    role, bypass = (torch.full((n,), 7, dtype=torch.int32, device="cuda:0") for _ in range(2))
    pi, pl, pp, pr_, pb = (host._ptr(t) for t in (index, label, path, role, bypass))
    assert L.dkmc_find_cuts(n, 2, pi, pl, None, 1, 1, pp, n, pr_, pb) == 0
    for args in ((-1, 2, pi, pl, None, 1, 1, pp, n, pr_, pb), (n, 0, pi, pl, None, 1, 1, pp, n, pr_, pb), (n, 2, pi, pl, None, 1, 1, pp, -1, pr_, pb),
                 (n, 2, pi, pl, None, 1, 1, pp, n + 1, pr_, pb), (n, 2, None, pl, None, 1, 1, pp, n, pr_, pb), (n, 2, pi, None, None, 1, 1, pp, n, pr_, pb),
                 (n, 2, pi, pl, None, 1, 1, None, n, pr_, pb), (n, 2, pi, pl, None, 1, 1, pp, n, None, pb), (n, 2, pi, pl, None, 1, 1, pp, n, pr_, None)):
        role.fill_(7); bypass.fill_(7)
        assert L.dkmc_find_cuts(*args) == 3
        assert "dkmc_find_cuts" in L.dkmc_last_error().decode()
        L.dkmc_clear_error()
        assert L.dkmc_get_cut_info(None) != 0                                       # no results of a failed call
        L.dkmc_clear_error()
        torch.cuda.synchronize()
        assert (role.cpu().numpy() == 7).all() and (bypass.cpu().numpy() == 7).all()       # nothing was launched
    assert L.dkmc_find_cuts(n, 2, pi, pl, None, 1, 1, None, 0, pr_, pb) == 0 and L.dkmc_get_cut_info(None) == 0     # d_path may be null with no rows


def test_getters_null_columns_and_capacity(hip):
    _, L = hip
    length = 5
    j = 2 * length
    n = 4 * length + 1
    links = ladder(length) + ladder(length, j + 1) + [(j - 2, j), (j - 1, j), (j, j + 1), (j, j + 2)]
    index, label, x = index_of(links, n), np.zeros(n, dtype=np.int32), np.arange(n) * 1.0
    path = pr.analyse(index, label, None, 2, 2, 0)[2]
    role, bypass, table, byp, necks, info = check_raw(hip, index, label, x, 2, 2, path)
    assert (len(table["site"]), len(byp["root"]), len(necks["first"])) == (2 * length + 1, 2, 1) and table["site"][table["cut"] == 1].tolist() == [j]
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    s, c, rows = np.full(16, -9, dtype=np.int32), np.full(16, -9, dtype=np.int32), C.c_int(-1)
    assert L.dkmc_copy_cut_path(4, vp(s), None, None, vp(c), C.byref(rows)) == 0 and rows.value == 4
    assert np.array_equal(s[:4], table["site"][:4]) and np.array_equal(c[:4], table["cut"][:4]) and (s[4:] == -9).all() and (c[4:] == -9).all()
    assert L.dkmc_copy_cut_path(0, None, None, None, None, C.byref(rows)) == 0 and rows.value == 0
    assert L.dkmc_copy_cut_path(10 ** 6, None, None, None, None, C.byref(rows)) == 0 and rows.value == 2 * length + 1
    assert L.dkmc_copy_cut_path(10 ** 6, None, None, None, None, None) == 0
    assert L.dkmc_copy_cut_path(-3, vp(s), None, None, None, C.byref(rows)) == 0 and rows.value == 0
    lo, hi = np.full(4, -9, dtype=np.int32), np.full(4, -9, dtype=np.int32)
    assert L.dkmc_copy_cut_bypasses(1, None, None, vp(lo), vp(hi), C.byref(rows)) == 0 and rows.value == 1
    assert (lo.tolist(), hi.tolist()) == ([-1, -9, -9, -9], [length, -9, -9, -9])
    assert L.dkmc_copy_cut_bypasses(4, None, None, vp(lo), None, C.byref(rows)) == 0 and rows.value == 2 and lo.tolist() == [-1, length, -9, -9]
    xmin, xmax = np.full(3, -9.0), np.full(3, -9.0)
    assert L.dkmc_copy_cut_necks(3, None, None, vp(xmin), vp(xmax), C.byref(rows)) == 0 and rows.value == 1
    assert (xmin.tolist(), xmax.tolist()) == ([float(j), -9.0, -9.0], [float(j), -9.0, -9.0])
    assert L.dkmc_copy_cut_necks(0, None, None, vp(xmin), None, None) == 0
    i16 = (C.c_longlong * 16)()
    assert L.dkmc_get_cut_info(i16) == 0 and list(i16) == [info[k] for k in cu.INFO] + [0, 0, 0, 0]


def test_two_calls_same_bytes(hip):
    rng = np.random.default_rng(21)
    N = 3000
    index, element, _, x = _random_case(rng, N, 6, 0.8, 0.6, False)
    label = np.where(element != 3, 0, -1).astype(np.int32)
    _, ptr, nb, sl, sr = cu.graph(index, label, 300, 300)
    path = cu.random_simple_path(rng, ptr, nb, sl, sr)
    assert len(path) > 0
    a = check_raw(hip, index, label, x, 300, 300, path)
    b = run_raw(hip, index, label, x, 300, 300, path)
    assert a[5]["status"] == 1 and _bytes(a) == _bytes(b)


# ---- the golden devices ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev_2p5(hip, cell_2p5):
    from devicekmc_amd import params as pm
    host, _ = hip
    p = pm.KMCParameters()
    dev = host.Device(cell_2p5, p)
    return dev, dev.make_gpubuf("cuda:0"), p, dev.site_element.copy()


class _Planted:
    """a planted filament in the device's site_element, taken out again on exit"""
    def __init__(self, dev, gb, el0, r):
        self.dev, self.gb, self.el0 = dev, gb, el0
        self.el2, _ = cr.plant_filament(el0, dev.site_x, dev.site_y, dev.site_z, r)

    def _set(self, el):
        import torch
        self.dev.site_element = el.copy()
        self.gb.t["site_element"].copy_(torch.as_tensor(el))

    def __enter__(self):
        self._set(self.el2)

    def __exit__(self, *exc):
        self._set(self.el0)


def _contacts(dev, p):
    return dev.get_num_in_contacts(p.num_atoms_first_layer, "left"), dev.get_num_in_contacts(p.num_atoms_first_layer, "right")


@pytest.mark.parametrize("r", [3.0, 2.6, 2.4, 2.2])
def test_planted_filaments_2p5(hip, dev_2p5, r):
    """Device.find_clusters -> Device.find_paths -> Device.find_cuts against the reference and the pinned figures"""
    dev, gb, p, el0 = dev_2p5
    with _Planted(dev, gb, el0, r):
        nl, nr = _contacts(dev, p)
        label, _, cinfo = dev.find_clusters(gb)
        _, _, path, _, pinfo = dev.find_paths(gb)
        res = dev.find_cuts(gb)
        role, bypass, table, byp, necks, info = res
        print(r, info)
        cu.assert_equal(*res, cu.analyse(dev.neigh_idx, label, dev.site_x, nl, nr, path))
        assert dev.site_role is role and dev.site_bypass is bypass and dev.cut_path is table and dev.cut_bypasses is byp and dev.cut_necks is necks
        assert dev.cut_info is info and pinfo["status"] == 1
        assert (info["path_len"], np.flatnonzero(table["cut"]).tolist(), info["necks"], info["longest_neck"], info["longest_neck_first"],
                info["bypasses"]) == PINNED_2P5[r]
        if r == 3.0:
            assert tuple(int(byp[k][0]) for k in cu.BYPASSES) == PINNED_2P5_WIDE_BYPASS
        # an empty path is the status 0 answer
        assert dev.find_cuts(gb, path=[])[5]["status"] == 0


def test_device_find_cuts_needs_labels_and_a_path(hip, dev_2p5, cell_2p5):
    host, _ = hip
    _, gb, p, _ = dev_2p5
    dev = host.Device(cell_2p5, p)
    with pytest.raises(ValueError, match="find_clusters"):
        dev.find_cuts(gb)
    dev.find_clusters(gb)
    with pytest.raises(ValueError, match="find_paths"):
        dev.find_cuts(gb)
    dev.find_paths(gb)                                                              # not bridged: an empty path
    assert dev.find_cuts(gb)[5]["status"] == 0


def test_wider_link_index_2p5(hip, dev_2p5):
    import torch
    host, _ = hip
    dev, gb, p, el0 = dev_2p5
    wide, nn = host.build_neighbor_index_gpu(dev.site_x, dev.site_y, dev.site_z, p.lattice, p.pbc, 5.0)
    with _Planted(dev, gb, el0, 2.2):
        nl, nr = _contacts(dev, p)
        link = (torch.as_tensor(wide.reshape(-1)).to("cuda:0"), nn)
        label, _, _ = dev.find_clusters(gb, link_index=link)
        _, _, path, _, pinfo = dev.find_paths(gb, link_index=link)
        res = dev.find_cuts(gb, link_index=link)
        assert pinfo["status"] == 1
        cu.assert_equal(*res, cu.analyse(wide, label, dev.site_x, nl, nr, path))


@pytest.mark.parametrize("r", [3.0, 2.2])
def test_planted_filament_7p5(hip, dev_7p5, r):
    host, _ = hip
    p = params_7p5()
    dev = host.Device(dev_7p5, p, gpu_neighbors="cuda:0")
    gb = dev.make_gpubuf("cuda:0")
    with _Planted(dev, gb, dev.site_element.copy(), r):
        nl, nr = _contacts(dev, p)
        label, _, _ = dev.find_clusters(gb)
        _, _, path, _, pinfo = dev.find_paths(gb)
        res = dev.find_cuts(gb)
        print(r, pinfo, res[5])
        assert pinfo["status"] == 1
        cu.assert_equal(*res, cu.analyse(dev.neigh_idx, label, dev.site_x, nl, nr, path))
