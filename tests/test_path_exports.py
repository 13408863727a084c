"""The conduction-path analysis (dkmc_find_paths): its four calls are declared and documented in the public header, exported by the built library
and bound in lib.py; the round cap and the times are debug aids; dkmc_stats keeps its layout; the snapshot writer's two hop columns.  No GPU: the
library is loaded, nothing is launched."""
import ctypes
import os
import re

import numpy as np
from analysis_support import _args, _code, _raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("dkmc_find_paths", "dkmc_get_path_info", "dkmc_copy_path_sites", "dkmc_copy_path_profile")
DEBUG = ("dkmc_debug_set_path_round_cap", "dkmc_debug_get_path_times")


def test_headers_declare_the_calls():
    pub, dbg = _code("devicekmc_hip.h"), _code("devicekmc_hip_debug.h")
    assert _args(pub, "dkmc_find_paths") == ["int N", "int nn", "const int *d_index", "const int *d_label", "const double *d_site_x", "int n_left_sites",
                                             "int n_right_sites", "int slack", "int *d_hops_left", "int *d_hops_right"]
    assert _args(pub, "dkmc_get_path_info") == ["long long *info8"]
    assert _args(pub, "dkmc_copy_path_sites") == ["int capacity", "int *h_site", "int *rows_out"]
    assert _args(pub, "dkmc_copy_path_profile") == ["int capacity", "int *h_count", "double *h_xmin", "double *h_xmax", "int *rows_out"]
    # the round cap and the times are debug aids: declared in the debug header, named nowhere in the public one
    assert re.search(r"\bvoid\s+dkmc_debug_set_path_round_cap\s*\(\s*int\s+\w+\s*\)\s*;", dbg)
    assert _args(dbg, "dkmc_debug_get_path_times") == ["double *ms2"]
    assert all(d not in _raw("devicekmc_hip.h") for d in DEBUG) and all(c not in dbg for c in CALLS)
    # after the gap block
    assert pub.index("dkmc_copy_gap_chain") < pub.index("dkmc_find_paths")


def test_header_documents_the_definitions():
    raw = _raw("devicekmc_hip.h")
    doc = raw[:raw.index("int dkmc_find_paths")]
    doc = doc[doc.rindex("/*"):]
    for word in ("members", "link", "seeds", "hops_left", "status", "slack", "corridor", "constriction", "rounds", "capacity", "rows_out", "NULL", "code 3"):
        assert word in doc, word
    # an addition: dkmc_stats keeps its layout
    body = re.sub(r"/\*.*?\*/", "", raw[raw.index("typedef struct dkmc_stats {"):raw.index("} dkmc_stats;")], flags=re.S)
    assert body.strip().rstrip(";").split()[-1] == "x_tile_f32_bytes"


def test_library_exports_and_lib_binds_the_calls():
    import __graft_entry__ as g
    g.build()
    from devicekmc_amd import host, lib
    L = lib.load()
    vp, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    assert lib.SYMBOLS["dkmc_find_paths"] == (I, [I, I, vp, vp, vp, I, I, I, vp, vp])
    assert lib.SYMBOLS["dkmc_get_path_info"] == (I, [ctypes.POINTER(ctypes.c_longlong)])
    assert lib.SYMBOLS["dkmc_copy_path_sites"] == (I, [I, vp, ctypes.POINTER(I)])
    assert lib.SYMBOLS["dkmc_copy_path_profile"] == (I, [I, vp, vp, vp, ctypes.POINTER(I)])
    assert lib.SYMBOLS["dkmc_debug_set_path_round_cap"] == (None, [I])
    assert lib.SYMBOLS["dkmc_debug_get_path_times"] == (I, [ctypes.POINTER(D)])
    for n in CALLS + DEBUG:
        assert hasattr(L, n), n
    assert lib.dkmc_stats._fields_[-1][0] == "x_tile_f32_bytes"
    assert callable(host.find_paths) and callable(host.Device.find_paths)
    assert host.PATH_INFO == ("status", "hops", "rounds", "reached_left", "reached_right", "corridor_sites", "constriction_level", "constriction_width")


def test_snapshot_hop_columns(tmp_path):
    from devicekmc_amd import io, params as pm
    el = np.array([pm.Ti_EL, pm.O_EL, pm.VACANCY, pm.Hf_EL, pm.N_EL], dtype=np.int32)
    x = np.array([0.0, 1.25, 2.5, 3.75, 5.0])
    y, z, pot, pw = x * 0.5, x * 0.25, np.linspace(0.0, 1.0, 5), np.array([0.0, 1e-9, 2.5e-7, 0.0, 3e-12])
    hl, hr = np.array([0, -1, 1, -1, 2], dtype=np.int32), np.array([2, -1, 1, -1, 0], dtype=np.int32)
    cl = np.array([0, -1, 0, -1, 0], dtype=np.int32)
    cur = np.array([1.5e-6, 0.0, 2.25e-7, 1e-12, 3.0e-6])
    for full in (False, True):
        f = (lambda v: repr(float(v))) if full else (lambda v: "%g" % v)
        a, b, c, d = (str(tmp_path / ("%s_%d.xyz" % (n, full))) for n in "abcd")
        # without them: the bytes of today's file, spelled out
        io.write_snapshot(a, el, x, y, z, pot, pw, full_precision=full)
        io.write_snapshot(b, el, x, y, z, pot, pw, full_precision=full, hops=None)
        want = "5\n\n" + "".join("   ".join([pm.ELEMENT_NAMES[int(el[i])], f(x[i]), f(y[i]), f(z[i]), f(pot[i]), f(pw[i])]) + "\n" for i in range(5))
        assert open(a, "rb").read() == want.encode() == open(b, "rb").read()
        # with them: two more integer columns, which read_xyz ignores
        io.write_snapshot(c, el, x, y, z, pot, pw, full_precision=full, hops=(hl, hr))
        lines = open(c).read().splitlines()[2:]
        rows = [l.split() for l in lines]
        assert all(len(r) == 8 for r in rows) and [int(r[6]) for r in rows] == hl.tolist() and [int(r[7]) for r in rows] == hr.tolist()
        assert [l.rsplit("   ", 2)[0] for l in lines] == want.splitlines()[2:]
        s = io.read_xyz(c)
        assert np.array_equal(s.element, el) and np.array_equal(s.x, x) and np.array_equal(s.y, y) and np.array_equal(s.z, z)
        # after current and cluster when all are given
        io.write_snapshot(d, el, x, y, z, pot, pw, full_precision=full, current=cur, cluster=cl, hops=(hl, hr))
        rows = [l.split() for l in open(d).read().splitlines()[2:]]
        assert all(len(r) == 10 for r in rows) and rows[0][6] == f(cur[0]) and [int(r[7]) for r in rows] == cl.tolist()
        assert [int(r[8]) for r in rows] == hl.tolist() and [int(r[9]) for r in rows] == hr.tolist()
        e = str(tmp_path / ("e_%d.xyz" % full))
        io.write_snapshot(e, el, x, y, z, pot, pw, full_precision=full, current=cur, cluster=cl)
        assert [l.rsplit("   ", 2)[0] for l in open(d).read().splitlines()][2:] == open(e).read().splitlines()[2:]
