"""dkmc_set_x_nmul_window, its test aid and its measurement aid: declared in the headers with the documented signatures and bound in lib.py.  No GPU:
nothing is loaded."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", " ", src, flags=re.S)                     # declarations only


def test_public_header_declares_the_switch():
    pub = _header("devicekmc_hip.h")
    assert re.search(r"\bvoid\s+dkmc_set_x_nmul_window\s*\(\s*int\s+\w+\s*\)\s*;", pub)
    assert re.search(r"\bint\s+dkmc_get_x_nmul_window\s*\(\s*void\s*\)\s*;", pub)


def test_debug_header_declares_the_aids():
    dbg = _header("devicekmc_hip_debug.h")
    assert re.search(r"\bvoid\s+dkmc_debug_set_x_nmul_window\s*\(\s*int\s+\w+\s*,\s*int\s+\w+\s*\)\s*;", dbg)
    assert re.search(r"\bint\s+dkmc_xtb_time_poly\s*\(\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*double\s*\*\s*\w+\s*\)\s*;", dbg)


def test_lib_binds_them():
    from devicekmc_amd import lib
    assert lib.SYMBOLS["dkmc_set_x_nmul_window"] == (None, [ctypes.c_int])
    assert lib.SYMBOLS["dkmc_get_x_nmul_window"] == (ctypes.c_int, [])
    assert lib.SYMBOLS["dkmc_debug_set_x_nmul_window"] == (None, [ctypes.c_int, ctypes.c_int])
    res, args = lib.SYMBOLS["dkmc_xtb_time_poly"]
    assert res is ctypes.c_int and len(args) == 3 and args[0] is ctypes.c_int and args[1] is ctypes.c_int


def test_the_library_exports_them():
    so = os.path.join(ROOT, "devicekmc_amd", "libdevicekmc_hip.so")
    if not os.path.exists(so):
        return                                                            # (not built here: the GPU tests load it)
    import subprocess
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    for name in ("dkmc_set_x_nmul_window", "dkmc_get_x_nmul_window", "dkmc_debug_set_x_nmul_window", "dkmc_xtb_time_poly"):
        assert re.search(r"\bT\s+%s\b" % name, syms), name
