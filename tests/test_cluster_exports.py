"""The filament analysis (dkmc_find_clusters): its three calls are declared in the public header, exported by the built library and bound in
lib.py, the round cap is a debug aid, and the snapshot writer's cluster column.  No GPU: the library is loaded, nothing is launched."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", " ", src, flags=re.S)


def test_headers_declare_the_calls():
    pub, dbg = _header("devicekmc_hip.h"), _header("devicekmc_hip_debug.h")
    m = re.search(r"\bint\s+dkmc_find_clusters\s*\(([^)]*)\)\s*;", pub)
    assert m and len(m.group(1).split(",")) == 12 and re.search(r"int\s*\*\s*d_label\s*$", m.group(1).strip())
    m = re.search(r"\bint\s+dkmc_copy_cluster_table\s*\(([^)]*)\)\s*;", pub)
    assert m and re.match(r"\s*int\s+capacity\b", m.group(1)) and len(m.group(1).split(",")) == 8
    assert re.search(r"\bint\s+dkmc_get_cluster_info\s*\(\s*int\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*\)\s*;", pub)
    assert re.search(r"\bvoid\s+dkmc_debug_set_cluster_round_cap\s*\(\s*int\s+\w+\s*\)\s*;", dbg) and "round_cap" not in pub
    raw = open(os.path.join(ROOT, "include", "devicekmc_hip.h")).read()
    doc = raw[:raw.index("int dkmc_find_clusters")]
    doc = doc[doc.rindex("/*"):]
    for word in ("members", "label", "n_left_sites", "bridge_root", "largest_free_size", "tip_left_x", "tip_right_x", "gap_x", "rounds", "capacity"):
        assert word in doc, word
    # an addition: dkmc_stats keeps its layout
    body = re.sub(r"/\*.*?\*/", "", raw[raw.index("typedef struct dkmc_stats {"):raw.index("} dkmc_stats;")], flags=re.S)
    assert body.strip().rstrip(";").split()[-1] == "x_tile_f32_bytes"


def test_library_exports_and_lib_binds_the_calls():
    import __graft_entry__ as g
    g.build()
    from devicekmc_amd import host, lib
    L = lib.load()
    vp, I = ctypes.c_void_p, ctypes.c_int
    assert lib.SYMBOLS["dkmc_find_clusters"] == (I, [I, I, vp, vp, vp, vp, vp, I, I, I, I, vp])
    assert lib.SYMBOLS["dkmc_copy_cluster_table"] == (I, [I, vp, vp, vp, vp, vp, vp, ctypes.POINTER(I)])
    assert lib.SYMBOLS["dkmc_get_cluster_info"] == (I, [ctypes.POINTER(I), ctypes.POINTER(ctypes.c_double)])
    assert lib.SYMBOLS["dkmc_debug_set_cluster_round_cap"] == (None, [I])
    for n in ("dkmc_find_clusters", "dkmc_copy_cluster_table", "dkmc_get_cluster_info", "dkmc_debug_set_cluster_round_cap"):
        assert hasattr(L, n), n
    assert lib.dkmc_stats._fields_[-1][0] == "x_tile_f32_bytes"
    assert (host.METAL, host.VACANCY, host.NEUTRAL_ONLY) == (1, 2, 4) and callable(host.Device.find_clusters)


def _sites():
    from devicekmc_amd import params as pm
    el = np.array([pm.Ti_EL, pm.O_EL, pm.VACANCY, pm.Hf_EL, pm.N_EL], dtype=np.int32)
    x = np.array([0.0, 1.25, 2.5, 3.75, 5.0])
    return el, x, x * 0.5, x * 0.25, np.linspace(0.0, 1.0, 5), np.array([0.0, 1e-9, 2.5e-7, 0.0, 3e-12])


def test_snapshot_cluster_column(tmp_path):
    from devicekmc_amd import io
    el, x, y, z, pot, pw = _sites()
    cl = np.array([0, -1, 0, -1, 4], dtype=np.int32)
    cur = np.array([1.5e-6, 0.0, 2.25e-7, 1e-12, 3.0e-6])
    for full in (False, True):
        f = (lambda v: repr(float(v))) if full else (lambda v: "%g" % v)
        a, b, c, d = (str(tmp_path / ("%s_%d.xyz" % (n, full))) for n in "abcd")
        # without it: the bytes of today's file, spelled out
        io.write_snapshot(a, el, x, y, z, pot, pw, full_precision=full)
        io.write_snapshot(b, el, x, y, z, pot, pw, full_precision=full, cluster=None)
        from devicekmc_amd.params import ELEMENT_NAMES
        want = "5\n\n" + "".join("   ".join([ELEMENT_NAMES[int(el[i])], f(x[i]), f(y[i]), f(z[i]), f(pot[i]), f(pw[i])]) + "\n" for i in range(5))
        assert open(a, "rb").read() == want.encode() == open(b, "rb").read()
        # with it: one more column, which read_xyz ignores
        io.write_snapshot(c, el, x, y, z, pot, pw, full_precision=full, cluster=cl)
        rows = [l.split() for l in open(c).read().splitlines()[2:]]
        assert all(len(r) == 7 for r in rows) and [int(r[6]) for r in rows] == cl.tolist()
        assert [l[:l.rindex("   ")] for l in open(c).read().splitlines()[2:]] == want.splitlines()[2:]
        s = io.read_xyz(c)
        assert np.array_equal(s.element, el) and np.array_equal(s.x, x) and np.array_equal(s.y, y) and np.array_equal(s.z, z)
        # after the current column when both are given
        io.write_snapshot(d, el, x, y, z, pot, pw, full_precision=full, current=cur, cluster=cl)
        rows = [l.split() for l in open(d).read().splitlines()[2:]]
        assert all(len(r) == 8 for r in rows) and [int(r[7]) for r in rows] == cl.tolist() and rows[0][6] == f(cur[0])
