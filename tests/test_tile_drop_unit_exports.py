"""dkmc_set_x_tile_drop_unit and its test aid: declared in the headers with the documented signatures and bound in lib.py.  No GPU: nothing is loaded."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", " ", src, flags=re.S)                     # declarations only


def test_public_header_declares_the_unit():
    pub = _header("devicekmc_hip.h")
    assert re.search(r"\bvoid\s+dkmc_set_x_tile_drop_unit\s*\(\s*int\s+\w+\s*\)\s*;", pub)
    assert re.search(r"\bint\s+dkmc_get_x_tile_drop_unit\s*\(\s*void\s*\)\s*;", pub)
    # the switch is an addition: dkmc_stats keeps its layout (its last field is still the fp32 image's size)
    raw = open(os.path.join(ROOT, "include", "devicekmc_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", raw[raw.index("typedef struct dkmc_stats {"):raw.index("} dkmc_stats;")], flags=re.S)
    assert body.strip().rstrip(";").split()[-1] == "x_tile_f32_bytes"


def test_debug_header_declares_the_masks():
    dbg = _header("devicekmc_hip_debug.h")
    assert re.search(r"\bint\s+dkmc_xt_get_live_masks\s*\(\s*double\s+\w+\s*,\s*int\s*\*\s*\w+\s*\)\s*;", dbg)


def test_lib_binds_the_unit_and_the_masks():
    from devicekmc_amd import lib
    assert lib.SYMBOLS["dkmc_set_x_tile_drop_unit"] == (None, [ctypes.c_int])
    assert lib.SYMBOLS["dkmc_get_x_tile_drop_unit"] == (ctypes.c_int, [])
    res, args = lib.SYMBOLS["dkmc_xt_get_live_masks"]
    assert res is ctypes.c_int and len(args) == 2 and args[0] is ctypes.c_double
