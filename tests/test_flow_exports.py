"""The min-cut analysis (dkmc_find_flow): its four calls are declared and documented in the public header, exported by the built library and
bound in lib.py; the round cap and the times are debug aids; dkmc_stats keeps its layout; the snapshot writer's zone column.  No GPU: the
library is loaded, nothing is launched."""
import ctypes
import os
import re

import numpy as np
from analysis_support import _args, _code, _raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("dkmc_find_flow", "dkmc_get_flow_info", "dkmc_copy_flow_strands", "dkmc_copy_flow_strand_sites")
DEBUG = ("dkmc_debug_set_flow_round_cap", "dkmc_debug_get_flow_times")


def test_headers_declare_the_calls():
    pub, dbg = _code("devicekmc_hip.h"), _code("devicekmc_hip_debug.h")
    assert _args(pub, "dkmc_find_flow") == ["int N", "int nn", "const int *d_index", "const int *d_label", "const double *d_site_x", "int n_left_sites",
                                            "int n_right_sites", "int max_strands", "int *d_site_zone", "int *d_site_strand"]
    assert _args(pub, "dkmc_get_flow_info") == ["long long *info16", "double *x4"]
    assert _args(pub, "dkmc_copy_flow_strands") == ["int capacity", "int *h_first_site", "int *h_last_site", "int *h_length", "int *h_offset",
                                                    "int *h_left_seed", "int *h_right_seed", "int *h_cut_left_site", "int *h_cut_left_pos",
                                                    "int *h_cut_right_site", "int *h_cut_right_pos", "int *rows_out"]
    assert _args(pub, "dkmc_copy_flow_strand_sites") == ["int capacity", "int *h_site", "int *rows_out"]
    # the zone bits have an enum, in the manner of DKMC_TRACK_*
    m = re.search(r"enum\s*\{([^}]*DKMC_FLOW_[^}]*)\}", pub)
    bits = dict((k.strip(), int(v)) for k, v in (e.split("=") for e in m.group(1).split(",")))
    assert bits == dict(DKMC_FLOW_MEMBER=1, DKMC_FLOW_LEFT_SHORE=2, DKMC_FLOW_LEFT_CUT=4, DKMC_FLOW_RIGHT_CUT=8, DKMC_FLOW_RIGHT_SHORE=16)
    # the round cap and the times are debug aids: declared in the debug header, named nowhere in the public one
    assert re.search(r"\bvoid\s+dkmc_debug_set_flow_round_cap\s*\(\s*int\s+\w+\s*\)\s*;", dbg)
    assert _args(dbg, "dkmc_debug_get_flow_times") == ["double *ms3"]
    assert all(d not in _raw("devicekmc_hip.h") for d in DEBUG) and all(c not in dbg for c in CALLS)
    # after the cut-site block, before the heat block
    assert pub.index("dkmc_copy_cut_necks") < pub.index("dkmc_find_flow") < pub.index("dkmc_copy_flow_strand_sites") < pub.index("dkmc_update_temperatureglobal_gpu")


def test_header_documents_the_definitions():
    raw = _raw("devicekmc_hip.h")
    doc = raw[:raw.index("int dkmc_find_flow")]
    doc = doc[doc.rindex("/*"):]
    for word in ("members", "link", "seeds", "interior", "near-left", "near-right", "strand", "disjoint", "contacts touch", "left-most minimum cut",
                 "right-most minimum cut", "left shore", "right shore", "in-node", "out-node", "residual", "exit", "smallest predecessor", "mirrored",
                 "max_strands", "status 3", "searches", "rounds", "closing round", "capacity", "rows_out", "NULL", "code 3", "4096"):
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
    assert lib.SYMBOLS["dkmc_find_flow"] == (I, [I, I, vp, vp, vp, I, I, I, vp, vp])
    assert lib.SYMBOLS["dkmc_get_flow_info"] == (I, [ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(D)])
    assert lib.SYMBOLS["dkmc_copy_flow_strands"] == (I, [I] + [vp] * 10 + [ctypes.POINTER(I)])
    assert lib.SYMBOLS["dkmc_copy_flow_strand_sites"] == (I, [I, vp, ctypes.POINTER(I)])
    assert lib.SYMBOLS["dkmc_debug_set_flow_round_cap"] == (None, [I])
    assert lib.SYMBOLS["dkmc_debug_get_flow_times"] == (I, [ctypes.POINTER(D)])
    for n in CALLS + DEBUG:
        assert hasattr(L, n), n
    assert lib.dkmc_stats._fields_[-1][0] == "x_tile_f32_bytes"
    assert callable(host.find_flow) and callable(host.Device.find_flow)
    import flow_ref as fl
    assert host.FLOW_INFO == fl.INFO and host.FLOW_STRANDS == fl.STRANDS and host.FLOW_ZONE == fl.ZONE
    assert host.FLOW_INFO[:2] == ("status", "width") and host.FLOW_INFO[8:10] == ("searches", "rounds") and len(host.FLOW_INFO) == 12
    assert [1 << k for k in range(len(host.FLOW_ZONE))] == [fl.MEMBER, fl.LEFT_SHORE, fl.LEFT_CUT, fl.RIGHT_CUT, fl.RIGHT_SHORE]


def test_argument_errors_launch_nothing_and_leave_the_getters_failing():
    """code 3 with the call's name before anything is launched (so: without a GPU), and no result is valid afterwards"""
    import __graft_entry__ as g
    g.build()
    from devicekmc_amd import lib
    L = lib.load()
    for args in ((-1, 1, None, None, None, 0, 0, 1, None, None), (0, 0, None, None, None, 0, 0, 1, None, None), (0, 1, None, None, None, 0, 0, 0, None, None),
                 (0, 1, None, None, None, 0, 0, 4097, None, None), (5, 1, None, None, None, 1, 1, 1, None, None)):
        assert L.dkmc_find_flow(*args) == 3
        assert b"dkmc_find_flow" in L.dkmc_last_error()
    rows = ctypes.c_int(-1)
    for call, args in ((L.dkmc_get_flow_info, (None, None)), (L.dkmc_copy_flow_strands, (0,) + (None,) * 10 + (ctypes.byref(rows),)),
                       (L.dkmc_copy_flow_strand_sites, (0, None, ctypes.byref(rows))), (L.dkmc_debug_get_flow_times, (None,))):
        assert call(*args) == 3
    L.dkmc_clear_error()


def test_snapshot_zone_column(tmp_path):
    from devicekmc_amd import io, params as pm
    el = np.array([pm.Ti_EL, pm.O_EL, pm.VACANCY, pm.Hf_EL, pm.N_EL], dtype=np.int32)
    x = np.array([0.0, 1.25, 2.5, 3.75, 5.0])
    y, z, pot, pw = x * 0.5, x * 0.25, np.linspace(0.0, 1.0, 5), np.array([0.0, 1e-9, 2.5e-7, 0.0, 3e-12])
    role = np.array([2, 0, 1, 0, 2], dtype=np.int32)
    zone = np.array([3, 0, 13, 0, 17], dtype=np.int32)
    for full in (False, True):
        f = (lambda v: repr(float(v))) if full else (lambda v: "%g" % v)
        a, b, c, d = (str(tmp_path / ("%s_%d.xyz" % (n, full))) for n in "abcd")
        # without it: the bytes of today's file, spelled out
        io.write_snapshot(a, el, x, y, z, pot, pw, full_precision=full)
        io.write_snapshot(b, el, x, y, z, pot, pw, full_precision=full, zone=None)
        want = "5\n\n" + "".join("   ".join([pm.ELEMENT_NAMES[int(el[i])], f(x[i]), f(y[i]), f(z[i]), f(pot[i]), f(pw[i])]) + "\n" for i in range(5))
        assert open(a, "rb").read() == want.encode() == open(b, "rb").read()
        # with it: one more integer column, which read_xyz ignores
        io.write_snapshot(c, el, x, y, z, pot, pw, full_precision=full, zone=zone)
        lines = open(c).read().splitlines()[2:]
        rows = [l.split() for l in lines]
        assert all(len(r) == 7 for r in rows) and [int(r[6]) for r in rows] == zone.tolist()
        assert [l.rsplit("   ", 1)[0] for l in lines] == want.splitlines()[2:]
        s = io.read_xyz(c)
        assert np.array_equal(s.element, el) and np.array_equal(s.x, x) and np.array_equal(s.y, y) and np.array_equal(s.z, z)
        # after the role column when both are given
        io.write_snapshot(d, el, x, y, z, pot, pw, full_precision=full, role=role, zone=zone)
        rows = [l.split() for l in open(d).read().splitlines()[2:]]
        assert all(len(r) == 8 for r in rows) and [int(r[6]) for r in rows] == role.tolist() and [int(r[7]) for r in rows] == zone.tolist()
        e = str(tmp_path / ("e_%d.xyz" % full))
        io.write_snapshot(e, el, x, y, z, pot, pw, full_precision=full, role=role)
        assert [l.rsplit("   ", 1)[0] for l in open(d).read().splitlines()][2:] == open(e).read().splitlines()[2:]
