"""The cut-site analysis (dkmc_find_cuts): its five calls are declared and documented in the public header, exported by the built library and
bound in lib.py; the round cap and the times are debug aids; dkmc_stats keeps its layout; the snapshot writer's role column.  No GPU: the library
is loaded, nothing is launched."""
import ctypes
import os
import re

import numpy as np
from analysis_support import _args, _code, _raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("dkmc_find_cuts", "dkmc_get_cut_info", "dkmc_copy_cut_path", "dkmc_copy_cut_bypasses", "dkmc_copy_cut_necks")
DEBUG = ("dkmc_debug_set_cut_round_cap", "dkmc_debug_get_cut_times")


def test_headers_declare_the_calls():
    pub, dbg = _code("devicekmc_hip.h"), _code("devicekmc_hip_debug.h")
    assert _args(pub, "dkmc_find_cuts") == ["int N", "int nn", "const int *d_index", "const int *d_label", "const double *d_site_x", "int n_left_sites",
                                            "int n_right_sites", "const int *d_path", "int path_len", "int *d_site_role", "int *d_site_bypass"]
    assert _args(pub, "dkmc_get_cut_info") == ["long long *info16"]
    assert _args(pub, "dkmc_copy_cut_path") == ["int capacity", "int *h_site", "int *h_n_bypass", "int *h_chord", "int *h_cut", "int *rows_out"]
    assert _args(pub, "dkmc_copy_cut_bypasses") == ["int capacity", "int *h_root", "int *h_size", "int *h_lo", "int *h_hi", "int *rows_out"]
    assert _args(pub, "dkmc_copy_cut_necks") == ["int capacity", "int *h_first", "int *h_last", "double *h_xmin", "double *h_xmax", "int *rows_out"]
    # the roles have an enum, in the manner of DKMC_TRACK_*
    m = re.search(r"enum\s*\{([^}]*DKMC_CUT_ROLE_[^}]*)\}", pub)
    roles = dict((k.strip(), int(v)) for k, v in (e.split("=") for e in m.group(1).split(",")))
    assert roles == dict(DKMC_CUT_ROLE_NONE=0, DKMC_CUT_ROLE_CUT=1, DKMC_CUT_ROLE_PATH=2, DKMC_CUT_ROLE_BYPASS=3, DKMC_CUT_ROLE_SIDE=4, DKMC_CUT_ROLE_APART=5)
    # the round cap and the times are debug aids: declared in the debug header, named nowhere in the public one
    assert re.search(r"\bvoid\s+dkmc_debug_set_cut_round_cap\s*\(\s*int\s+\w+\s*\)\s*;", dbg)
    assert _args(dbg, "dkmc_debug_get_cut_times") == ["double *ms2"]
    assert all(d not in _raw("devicekmc_hip.h") for d in DEBUG) and all(c not in dbg for c in CALLS)
    # after the tracking block, before the heat block
    assert pub.index("dkmc_copy_track_critical") < pub.index("dkmc_find_cuts") < pub.index("dkmc_copy_cut_necks") < pub.index("dkmc_update_temperatureglobal_gpu")


def test_header_documents_the_definitions():
    raw = _raw("devicekmc_hip.h")
    doc = raw[:raw.index("int dkmc_find_cuts")]
    doc = doc[doc.rindex("/*"):]
    for word in ("members", "link", "seeds", "cut site", "off-path", "attachment", "chord", "bypass", "neck", "rounds", "capacity", "rows_out", "NULL",
                 "code 3"):
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
    assert lib.SYMBOLS["dkmc_find_cuts"] == (I, [I, I, vp, vp, vp, I, I, vp, I, vp, vp])
    assert lib.SYMBOLS["dkmc_get_cut_info"] == (I, [ctypes.POINTER(ctypes.c_longlong)])
    assert lib.SYMBOLS["dkmc_copy_cut_path"] == (I, [I, vp, vp, vp, vp, ctypes.POINTER(I)])
    assert lib.SYMBOLS["dkmc_copy_cut_bypasses"] == (I, [I, vp, vp, vp, vp, ctypes.POINTER(I)])
    assert lib.SYMBOLS["dkmc_copy_cut_necks"] == (I, [I, vp, vp, vp, vp, ctypes.POINTER(I)])
    assert lib.SYMBOLS["dkmc_debug_set_cut_round_cap"] == (None, [I])
    assert lib.SYMBOLS["dkmc_debug_get_cut_times"] == (I, [ctypes.POINTER(D)])
    for n in CALLS + DEBUG:
        assert hasattr(L, n), n
    assert lib.dkmc_stats._fields_[-1][0] == "x_tile_f32_bytes"
    assert callable(host.find_cuts) and callable(host.Device.find_cuts)
    assert host.CUT_INFO == ("status", "path_len", "cut_sites", "necks", "longest_neck", "longest_neck_first", "bypasses", "offpath_components",
                             "offpath_members", "max_bypass", "chord_positions", "rounds")
    import cut_ref as cu
    assert host.CUT_INFO == cu.INFO and host.CUT_PATH == cu.PATH and host.CUT_BYPASSES == cu.BYPASSES and host.CUT_NECKS == cu.NECKS
    assert len(host.CUT_ROLE) == 6 and host.CUT_ROLE[cu.CUT] == "cut" and host.CUT_ROLE[cu.APART] == "apart"


def test_snapshot_role_column(tmp_path):
    from devicekmc_amd import io, params as pm
    el = np.array([pm.Ti_EL, pm.O_EL, pm.VACANCY, pm.Hf_EL, pm.N_EL], dtype=np.int32)
    x = np.array([0.0, 1.25, 2.5, 3.75, 5.0])
    y, z, pot, pw = x * 0.5, x * 0.25, np.linspace(0.0, 1.0, 5), np.array([0.0, 1e-9, 2.5e-7, 0.0, 3e-12])
    hl, hr = np.array([0, -1, 1, -1, 2], dtype=np.int32), np.array([2, -1, 1, -1, 0], dtype=np.int32)
    role = np.array([2, 0, 1, 0, 2], dtype=np.int32)
    for full in (False, True):
        f = (lambda v: repr(float(v))) if full else (lambda v: "%g" % v)
        a, b, c, d = (str(tmp_path / ("%s_%d.xyz" % (n, full))) for n in "abcd")
        # without it: the bytes of today's file, spelled out
        io.write_snapshot(a, el, x, y, z, pot, pw, full_precision=full)
        io.write_snapshot(b, el, x, y, z, pot, pw, full_precision=full, role=None)
        want = "5\n\n" + "".join("   ".join([pm.ELEMENT_NAMES[int(el[i])], f(x[i]), f(y[i]), f(z[i]), f(pot[i]), f(pw[i])]) + "\n" for i in range(5))
        assert open(a, "rb").read() == want.encode() == open(b, "rb").read()
        # with it: one more integer column, which read_xyz ignores
        io.write_snapshot(c, el, x, y, z, pot, pw, full_precision=full, role=role)
        lines = open(c).read().splitlines()[2:]
        rows = [l.split() for l in lines]
        assert all(len(r) == 7 for r in rows) and [int(r[6]) for r in rows] == role.tolist()
        assert [l.rsplit("   ", 1)[0] for l in lines] == want.splitlines()[2:]
        s = io.read_xyz(c)
        assert np.array_equal(s.element, el) and np.array_equal(s.x, x) and np.array_equal(s.y, y) and np.array_equal(s.z, z)
        # after the hop columns when both are given
        io.write_snapshot(d, el, x, y, z, pot, pw, full_precision=full, hops=(hl, hr), role=role)
        rows = [l.split() for l in open(d).read().splitlines()[2:]]
        assert all(len(r) == 9 for r in rows) and [int(r[6]) for r in rows] == hl.tolist() and [int(r[7]) for r in rows] == hr.tolist()
        assert [int(r[8]) for r in rows] == role.tolist()
        e = str(tmp_path / ("e_%d.xyz" % full))
        io.write_snapshot(e, el, x, y, z, pot, pw, full_precision=full, hops=(hl, hr))
        assert [l.rsplit("   ", 1)[0] for l in open(d).read().splitlines()][2:] == open(e).read().splitlines()[2:]
