"""The current map (dkmc_set_current_map): its four calls are declared in the public header with the documented signatures and bound in lib.py;
the snapshot writer's extra column; the plane profile of the signed tunnelling outflow.  No GPU: nothing is loaded."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", " ", src, flags=re.S)                     # declarations only


def test_public_header_declares_the_four_calls():
    pub = _header("devicekmc_hip.h")
    buf, dbl = r"const\s+dkmc_gpubuf\s*\*\s*\w+", r"double\s*\*\s*\w+"
    assert re.search(r"\bvoid\s+dkmc_set_current_map\s*\(\s*int\s+\w+\s*\)\s*;", pub)
    assert re.search(r"\bint\s+dkmc_get_current_map\s*\(\s*void\s*\)\s*;", pub)
    assert re.search(r"\bint\s+dkmc_copy_current_map_from_gpu\s*\(\s*%s\s*,\s*%s\s*,\s*%s\s*,\s*%s\s*\)\s*;" % (buf, dbl, dbl, dbl), pub)
    assert re.search(r"\bint\s+dkmc_get_current_map_info\s*\(\s*%s\s*,\s*%s\s*\)\s*;" % (buf, dbl), pub)
    # ... with the definitions in the comment in front of them
    raw = open(os.path.join(ROOT, "include", "devicekmc_hip.h")).read()
    doc = raw[:raw.index("void dkmc_set_current_map")]
    doc = doc[doc.rindex("/*"):]
    for word in ("thr_all", "thr_tun", "net_tun", "info8", "J_ic"):
        assert word in doc, word
    # the feature is an addition: dkmc_stats keeps its layout (its last field is still the fp32 image's size)
    body = re.sub(r"/\*.*?\*/", "", raw[raw.index("typedef struct dkmc_stats {"):raw.index("} dkmc_stats;")], flags=re.S)
    assert body.strip().rstrip(";").split()[-1] == "x_tile_f32_bytes"


def test_lib_binds_the_four_calls():
    from devicekmc_amd import lib
    assert lib.SYMBOLS["dkmc_set_current_map"] == (None, [ctypes.c_int])
    assert lib.SYMBOLS["dkmc_get_current_map"] == (ctypes.c_int, [])
    res, args = lib.SYMBOLS["dkmc_copy_current_map_from_gpu"]
    assert res is ctypes.c_int and len(args) == 4 and args[0] == ctypes.POINTER(lib.dkmc_gpubuf)
    res, args = lib.SYMBOLS["dkmc_get_current_map_info"]
    assert res is ctypes.c_int and len(args) == 2 and args[0] == ctypes.POINTER(lib.dkmc_gpubuf) and args[1] == ctypes.POINTER(ctypes.c_double)
    assert lib.dkmc_stats._fields_[-1][0] == "x_tile_f32_bytes"


def _sites():
    from devicekmc_amd import params as pm
    el = np.array([pm.Ti_EL, pm.O_EL, pm.VACANCY, pm.Hf_EL, pm.N_EL], dtype=np.int32)
    x = np.array([0.0, 1.25, 2.5, 3.75, 5.0]); y = x * 0.5; z = x * 0.25
    return el, x, y, z, np.linspace(0.0, 1.0, 5), np.array([0.0, 1e-9, 2.5e-7, 0.0, 3e-12])


def test_snapshot_current_column_round_trips(tmp_path):
    from devicekmc_amd import io
    el, x, y, z, pot, pw = _sites()
    cur = np.array([1.5e-6, 0.0, 2.25e-7, 1e-12, 3.0e-6])
    for full in (False, True):
        path = str(tmp_path / ("snap_%d.xyz" % full))
        io.write_snapshot(path, el, x, y, z, pot, pw, full_precision=full, current=cur)
        s = io.read_xyz(path)                                  # the reader ignores the extra column
        assert np.array_equal(s.element, el) and np.array_equal(s.x, x) and np.array_equal(s.y, y) and np.array_equal(s.z, z)
        rows = [l.split() for l in open(path).read().splitlines()[2:]]
        assert all(len(r) == 7 for r in rows)
        col = np.array([float(r[6]) for r in rows])
        assert np.array_equal(col, cur) if full else np.allclose(col, cur, rtol=1e-5, atol=0.0)
        assert rows[0][6] == (repr(1.5e-6) if full else "1.5e-06")


def test_snapshot_without_current_is_unchanged(tmp_path):
    from devicekmc_amd import io
    el, x, y, z, pot, pw = _sites()
    for full in (False, True):
        a, b = str(tmp_path / ("a_%d.xyz" % full)), str(tmp_path / ("b_%d.xyz" % full))
        io.write_snapshot(a, el, x, y, z, pot, pw, full_precision=full)
        io.write_snapshot(b, el, x, y, z, pot, pw, full_precision=full, current=None)
        data = open(a, "rb").read()
        assert data == open(b, "rb").read()
        lines = data.decode().splitlines()
        assert lines[0] == "5" and lines[1] == "" and all(len(l.split()) == 6 for l in lines[2:])
        # the reference's format: three blanks between the six fields
        from devicekmc_amd.params import ELEMENT_NAMES
        f = (lambda v: repr(float(v))) if full else (lambda v: "%g" % v)
        assert lines[3] == "   ".join([ELEMENT_NAMES[int(el[1])], f(x[1]), f(y[1]), f(z[1]), f(pot[1]), f(pw[1])])


def test_tunnel_current_profile_is_the_cumulative_outflow():
    from devicekmc_amd import host

    class Dev:
        tunnel_current_profile = host.Device.tunnel_current_profile

    d = Dev()
    d.site_x = np.array([3.0, 1.0, 2.0, 5.0, 4.0, 2.0])
    d.site_tunnel_outflow = np.array([0.5, 2.0, -0.25, -3.0, 1.0, -0.25])
    got = d.tunnel_current_profile([0.0, 1.0, 2.0, 3.5, 4.0, 10.0])
    assert np.array_equal(got, np.array([0.0, 2.0, 1.5, 2.0, 3.0, 0.0]))      # below every site: 0; above every site: the total
    assert got[-1] == d.site_tunnel_outflow.sum()
    assert np.array_equal(d.tunnel_current_profile(2.0), np.array([1.5]))
