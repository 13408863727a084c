"""The switch between the two forms of the pair sum's kernels (dkmc_set_pair_form) and the report of the last profiled call
(dkmc_get_pair_sum_info): declared in the right headers, bound in lib.py, and dkmc_stats untouched (no GPU needed)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _text(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_headers_declare_the_pair_form_functions():
    pub, dbg = _text("include", "devicekmc_hip.h"), _text("include", "devicekmc_hip_debug.h")
    assert re.search(r"\bvoid\s+dkmc_set_pair_form\s*\(\s*int\s+\w+\s*\)\s*;", pub)
    assert re.search(r"\bint\s+dkmc_get_pair_form\s*\(\s*void\s*\)\s*;", pub)
    assert re.search(r"\bint\s+dkmc_get_pair_sum_info\s*\(\s*long long\s*\*\s*\w+\s*(/\*.*?\*/)?\s*,\s*double\s*\*\s*\w+\s*(/\*.*?\*/)?\s*\)\s*;", dbg)
    assert "dkmc_get_pair_sum_info" not in pub         # a measurement aid, not part of the surface


def test_lib_binds_them_with_these_signatures():
    from devicekmc_amd import lib
    assert lib.SYMBOLS["dkmc_set_pair_form"] == (None, [C.c_int])
    assert lib.SYMBOLS["dkmc_get_pair_form"] == (C.c_int, [])
    assert lib.SYMBOLS["dkmc_get_pair_sum_info"] == (C.c_int, [C.POINTER(C.c_longlong), C.POINTER(C.c_double)])


def test_stats_still_end_with_the_tile_fields():
    from devicekmc_amd import lib
    assert [f[0] for f in lib.dkmc_stats._fields_][-3:] == ["x_tile_stream", "x_tile_f64_rounds", "x_tile_f32_bytes"]
    names = [f[0] for f in lib.dkmc_stats._fields_]
    assert "pair_evaluated" in names and "pair_tested" in names and "pair_ms" in names
