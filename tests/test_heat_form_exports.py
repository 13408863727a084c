"""The switch of the local heat model (dkmc_set_heat_form), its report and its test aid: declared, bound and off by default (no GPU needed)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _text(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_headers_declare_the_heat_form_functions():
    pub, dbg = _text("include", "devicekmc_hip.h"), _text("include", "devicekmc_hip_debug.h")
    assert re.search(r"\bvoid\s+dkmc_set_heat_form\s*\(\s*int\s+\w+\s*\)\s*;", pub)
    assert re.search(r"\bint\s+dkmc_get_heat_form\s*\(\s*void\s*\)\s*;", pub)
    assert re.search(r"\bint\s+dkmc_get_heat_info\s*\(\s*long long\s*\*\s*\w+\s*\)\s*;", pub)
    assert re.search(r"\bvoid\s+dkmc_debug_heat_chain\s*\(\s*int\s+\w+\s*,\s*int\s+\w+\s*\)\s*;", dbg)
    assert "dkmc_debug_heat_chain" not in pub          # a test aid, not part of the surface


def test_lib_binds_them_and_the_default_is_off():
    import ctypes as C
    from devicekmc_amd import lib
    assert lib.SYMBOLS["dkmc_set_heat_form"] == (None, [C.c_int])
    assert lib.SYMBOLS["dkmc_get_heat_form"] == (C.c_int, [])
    assert lib.SYMBOLS["dkmc_get_heat_info"] == (C.c_int, [C.POINTER(C.c_longlong)])
    assert lib.SYMBOLS["dkmc_debug_heat_chain"] == (None, [C.c_int, C.c_int])
    if os.path.exists(lib.LIB_PATH):
        # host code only: the switch touches no GPU (every test that flips it resets it in a `finally`)
        L = lib.load()
        assert L.dkmc_get_heat_form() == 0
        try:
            L.dkmc_set_heat_form(7)
            assert L.dkmc_get_heat_form() == 1
        finally:
            L.dkmc_set_heat_form(0)
        assert L.dkmc_get_heat_form() == 0
        info = (C.c_longlong * 8)()
        assert L.dkmc_get_heat_info(info) == 0 and info[7] == 0
