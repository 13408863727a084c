"""The cluster tracking (dkmc_track_clusters): its six calls are declared and documented in the public header, exported by the built library and
bound in lib.py; the hash mode and the times are debug aids; dkmc_stats keeps its layout; the snapshot writer's change column.  No GPU: the
library is loaded, nothing is launched."""
import ctypes
import os
import re

import numpy as np
from analysis_support import _args, _code, _raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("dkmc_track_clusters", "dkmc_get_track_info", "dkmc_copy_track_pairs", "dkmc_copy_track_now", "dkmc_copy_track_prev", "dkmc_copy_track_critical")
DEBUG = ("dkmc_debug_set_track_hash", "dkmc_debug_get_track_times")


def test_headers_declare_the_calls():
    pub, dbg = _code("devicekmc_hip.h"), _code("devicekmc_hip_debug.h")
    assert _args(pub, "dkmc_track_clusters") == ["int N", "const int *d_label_prev", "const int *d_label_now", "const double *d_site_x", "int n_left_sites",
                                                 "int n_right_sites", "int *d_site_change"]
    assert _args(pub, "dkmc_get_track_info") == ["long long *info16", "double *x2"]
    assert _args(pub, "dkmc_copy_track_pairs") == ["int capacity", "int *h_prev", "int *h_now", "int *h_count", "int *h_first_site", "int *rows_out"]
    assert _args(pub, "dkmc_copy_track_now") == ["int capacity", "int *h_root", "int *h_size", "int *h_joined", "int *h_n_parents", "int *h_main_parent",
                                                 "int *h_flags", "int *rows_out"]
    assert _args(pub, "dkmc_copy_track_prev") == ["int capacity", "int *h_root", "int *h_size", "int *h_left", "int *h_n_children", "int *h_main_child",
                                                  "int *h_flags", "int *rows_out"]
    assert _args(pub, "dkmc_copy_track_critical") == ["int capacity", "int *h_site", "int *rows_out"]
    # the hash mode and the times are debug aids: declared in the debug header, named nowhere in the public one
    assert re.search(r"\bvoid\s+dkmc_debug_set_track_hash\s*\(\s*int\s+\w+\s*\)\s*;", dbg)
    assert _args(dbg, "dkmc_debug_get_track_times") == ["double *ms2"]
    assert all(d not in _raw("devicekmc_hip.h") for d in DEBUG) and all(c not in dbg for c in CALLS)
    # after the path block, before the temperature calls
    assert pub.index("dkmc_copy_path_profile") < pub.index("dkmc_track_clusters") < pub.index("dkmc_copy_track_critical") < pub.index("dkmc_update_temperatureglobal_gpu")


def test_header_documents_the_definitions():
    raw = _raw("devicekmc_hip.h")
    doc = raw[:raw.index("int dkmc_track_clusters")]
    doc = doc[doc.rindex("/*"):]
    for word in ("sides", "site_change", "joined", "left", "regrouped", "main line", "pairs", "first_site", "now table", "prev table", "n_parents", "main_parent",
                 "n_children", "main_child", "BORN", "DIED", "MERGED", "SPLIT", "FRAGMENT", "ABSORBED", "verdicts", "bridge_prev", "bridge_now", "transition",
                 "critical", "x2", "info16", "capacity", "rows_out", "NULL", "code 3", "same pointer"):
        assert word in doc, word
    # an addition: dkmc_stats keeps its layout
    body = re.sub(r"/\*.*?\*/", "", raw[raw.index("typedef struct dkmc_stats {"):raw.index("} dkmc_stats;")], flags=re.S)
    assert body.strip().rstrip(";").split()[-1] == "x_tile_f32_bytes"


def test_library_exports_and_lib_binds_the_calls():
    import __graft_entry__ as g
    g.build()
    from devicekmc_amd import host, lib
    L = lib.load()
    vp, I, D, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_longlong
    assert lib.SYMBOLS["dkmc_track_clusters"] == (I, [I, vp, vp, vp, I, I, vp])
    assert lib.SYMBOLS["dkmc_get_track_info"] == (I, [ctypes.POINTER(LL), ctypes.POINTER(D)])
    assert lib.SYMBOLS["dkmc_copy_track_pairs"] == (I, [I, vp, vp, vp, vp, ctypes.POINTER(I)])
    assert lib.SYMBOLS["dkmc_copy_track_now"] == (I, [I, vp, vp, vp, vp, vp, vp, ctypes.POINTER(I)])
    assert lib.SYMBOLS["dkmc_copy_track_prev"] == (I, [I, vp, vp, vp, vp, vp, vp, ctypes.POINTER(I)])
    assert lib.SYMBOLS["dkmc_copy_track_critical"] == (I, [I, vp, ctypes.POINTER(I)])
    assert lib.SYMBOLS["dkmc_debug_set_track_hash"] == (None, [I])
    assert lib.SYMBOLS["dkmc_debug_get_track_times"] == (I, [ctypes.POINTER(D)])
    for n in CALLS + DEBUG:
        assert hasattr(L, n), n
    assert lib.dkmc_stats._fields_[-1][0] == "x_tile_f32_bytes"
    assert callable(host.track_clusters) and callable(host.Device.track_clusters)
    assert host.TRACK_INFO == ("n_prev", "n_now", "n_pairs", "stayed", "joined", "left", "regrouped", "transition", "bridge_prev", "bridge_now",
                               "born", "died", "merged", "split", "n_critical")
    assert host.TRACK_PAIRS == ("prev", "now", "count", "first_site")
    assert host.TRACK_NOW == ("root", "size", "joined", "n_parents", "main_parent", "flags")
    assert host.TRACK_PREV == ("root", "size", "left", "n_children", "main_child", "flags")
    assert host.TRACK_CHANGE == ("none", "stayed", "joined", "left", "regrouped")
    # the reference of the tests restates the same names and bits
    import track_ref as tr
    assert (tr.INFO, tr.PAIRS, tr.NOW, tr.PREV) == (host.TRACK_INFO, host.TRACK_PAIRS, host.TRACK_NOW, host.TRACK_PREV)
    assert (tr.BORN, tr.MERGED, tr.FRAGMENT, tr.DIED, tr.SPLIT, tr.ABSORBED) == (host.TRACK_BORN, host.TRACK_MERGED, host.TRACK_FRAGMENT, host.TRACK_DIED,
                                                                                host.TRACK_SPLIT, host.TRACK_ABSORBED)
    assert [host.TRACK_CHANGE[c] for c in (tr.NONE, tr.STAYED, tr.JOINED, tr.LEFT_, tr.REGROUPED)] == list(host.TRACK_CHANGE)


def test_device_track_clusters_needs_two_labellings():
    """raised before anything touches the device"""
    import pytest
    from devicekmc_amd import host
    dev = object.__new__(host.Device)
    with pytest.raises(ValueError, match="fewer than two"):
        dev.track_clusters(None)
    dev._cluster_label_prev, dev._cluster_label = None, object()            # one find_clusters call so far
    with pytest.raises(ValueError, match="fewer than two"):
        dev.track_clusters(None)


def test_snapshot_change_column(tmp_path):
    from devicekmc_amd import io, params as pm
    el = np.array([pm.Ti_EL, pm.O_EL, pm.VACANCY, pm.Hf_EL, pm.N_EL], dtype=np.int32)
    x = np.array([0.0, 1.25, 2.5, 3.75, 5.0])
    y, z, pot, pw = x * 0.5, x * 0.25, np.linspace(0.0, 1.0, 5), np.array([0.0, 1e-9, 2.5e-7, 0.0, 3e-12])
    hl, hr = np.array([0, -1, 1, -1, 2], dtype=np.int32), np.array([2, -1, 1, -1, 0], dtype=np.int32)
    cl = np.array([0, -1, 0, -1, 0], dtype=np.int32)
    cur = np.array([1.5e-6, 0.0, 2.25e-7, 1e-12, 3.0e-6])
    ch = np.array([1, 0, 2, 3, 4], dtype=np.int32)
    for full in (False, True):
        f = (lambda v: repr(float(v))) if full else (lambda v: "%g" % v)
        a, b, c, d, e = (str(tmp_path / ("%s_%d.xyz" % (n, full))) for n in "abcde")
        # without it: the bytes of today's file, spelled out
        io.write_snapshot(a, el, x, y, z, pot, pw, full_precision=full)
        io.write_snapshot(b, el, x, y, z, pot, pw, full_precision=full, change=None)
        want = "5\n\n" + "".join("   ".join([pm.ELEMENT_NAMES[int(el[i])], f(x[i]), f(y[i]), f(z[i]), f(pot[i]), f(pw[i])]) + "\n" for i in range(5))
        assert open(a, "rb").read() == want.encode() == open(b, "rb").read()
        # with it: one more integer column, which read_xyz ignores
        io.write_snapshot(c, el, x, y, z, pot, pw, full_precision=full, change=ch)
        lines = open(c).read().splitlines()[2:]
        rows = [l.split() for l in lines]
        assert all(len(r) == 7 for r in rows) and [int(r[6]) for r in rows] == ch.tolist()
        assert [l.rsplit("   ", 1)[0] for l in lines] == want.splitlines()[2:]
        s = io.read_xyz(c)
        assert np.array_equal(s.element, el) and np.array_equal(s.x, x) and np.array_equal(s.y, y) and np.array_equal(s.z, z)
        # the last column, after current, cluster and hops, when all are given; the columns before it are the file without it
        io.write_snapshot(d, el, x, y, z, pot, pw, full_precision=full, current=cur, cluster=cl, hops=(hl, hr), change=ch)
        io.write_snapshot(e, el, x, y, z, pot, pw, full_precision=full, current=cur, cluster=cl, hops=(hl, hr))
        rows = [l.split() for l in open(d).read().splitlines()[2:]]
        assert all(len(r) == 11 for r in rows) and rows[0][6] == f(cur[0]) and [int(r[7]) for r in rows] == cl.tolist()
        assert [int(r[8]) for r in rows] == hl.tolist() and [int(r[9]) for r in rows] == hr.tolist() and [int(r[10]) for r in rows] == ch.tolist()
        assert [l.rsplit("   ", 1)[0] for l in open(d).read().splitlines()][2:] == open(e).read().splitlines()[2:]
