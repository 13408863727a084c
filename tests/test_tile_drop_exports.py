"""dkmc_set_x_tile_drop, its report and its test aids: declared in the headers with the documented signatures and bound in lib.py.  No GPU: nothing
is loaded."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", " ", src, flags=re.S)                     # declarations only


def test_public_header_declares_the_switch():
    pub = _header("devicekmc_hip.h")
    assert re.search(r"\bvoid\s+dkmc_set_x_tile_drop\s*\(\s*double\s+\w+\s*\)\s*;", pub)
    assert re.search(r"\bdouble\s+dkmc_get_x_tile_drop\s*\(\s*void\s*\)\s*;", pub)
    # the switch is an addition: dkmc_stats keeps its layout (its last field is still the fp32 image's size)
    raw = open(os.path.join(ROOT, "include", "devicekmc_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", raw[raw.index("typedef struct dkmc_stats {"):raw.index("} dkmc_stats;")], flags=re.S)
    assert body.strip().rstrip(";").split()[-1] == "x_tile_f32_bytes"


def test_lib_binds_the_switch_and_the_aids():
    from devicekmc_amd import lib
    assert lib.SYMBOLS["dkmc_set_x_tile_drop"] == (None, [ctypes.c_double])
    assert lib.SYMBOLS["dkmc_get_x_tile_drop"] == (ctypes.c_double, [])
    res, args = lib.SYMBOLS["dkmc_get_x_tile_live_info"]
    assert res is ctypes.c_int and len(args) == 2 and args[0] == ctypes.POINTER(ctypes.c_longlong) and args[1] == ctypes.POINTER(ctypes.c_double)
    res, args = lib.SYMBOLS["dkmc_xt_get_live"]
    assert res is ctypes.c_int and len(args) == 3 and args[0] is ctypes.c_double


def test_debug_header_declares_the_three_aids():
    dbg = _header("devicekmc_hip_debug.h")
    assert re.search(r"\bint\s+dkmc_get_x_tile_live_info\s*\(\s*long\s+long\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*\)\s*;", dbg)
    assert re.search(r"\bint\s+dkmc_xt_get_live\s*\(\s*double\s+\w+\s*,\s*int\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*\)\s*;", dbg)
    assert re.search(r"\bint\s+dkmc_xtb_tile_product\s*\(\s*int\s+\w+\s*,\s*int\s+stored_bytes\s*,\s*double\s*\*\s*\w+\s*\)\s*;", dbg)
    # ... and documents the live image as a value of stored_bytes
    raw = open(os.path.join(ROOT, "include", "devicekmc_hip_debug.h")).read()
    doc = raw[:raw.index("int dkmc_xtb_tile_product")]
    assert "stored_bytes -4" in doc[doc.rindex("/*"):]
