"""The gap analysis (dkmc_find_gaps): its four calls are declared and documented in the public header, exported by the built library and bound in
lib.py; the uniform-cell skip is a debug aid; dkmc_stats keeps its layout.  No GPU: the library is loaded, nothing is launched."""
import ctypes
import os
import re
from analysis_support import _args, _code, _raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("dkmc_find_gaps", "dkmc_get_gap_info", "dkmc_copy_gap_edges", "dkmc_copy_gap_chain")


def test_headers_declare_the_calls():
    pub, dbg = _code("devicekmc_hip.h"), _code("devicekmc_hip_debug.h")
    assert _args(pub, "dkmc_find_gaps") == ["int N", "const double *d_x", "const double *d_y", "const double *d_z", "const double *h_lattice", "int pbc",
                                            "const int *d_label", "int n_left_sites", "int n_right_sites", "double r_max"]
    assert _args(pub, "dkmc_get_gap_info") == ["long long *info8", "double *d2x2"]
    assert _args(pub, "dkmc_copy_gap_edges") == ["int capacity", "int *h_site_a", "int *h_site_b", "int *h_root_a", "int *h_root_b", "double *h_d2", "int *rows_out"]
    assert _args(pub, "dkmc_copy_gap_chain") == ["int capacity", "int *h_from", "int *h_to", "double *h_d2", "int *rows_out"]
    # the uniform-cell skip is a debug switch: declared in the debug header, named nowhere in the public one
    assert re.search(r"\bvoid\s+dkmc_debug_set_gap_cell_skip\s*\(\s*int\s+\w+\s*\)\s*;", dbg)
    assert "cell_skip" not in pub and all(c not in dbg for c in CALLS)


def test_header_documents_the_definitions():
    raw = _raw("devicekmc_hip.h")
    doc = raw[:raw.index("int dkmc_find_gaps")]
    doc = doc[doc.rindex("/*"):]
    for word in ("members", "d_label", "n_left_sites", "n_right_sites", "bridged", "min(u, v)", "round(fy)", "lattice[1]", "(d2, a, b)", "r_max * r_max",
                 "minimum spanning forest", "site_a < site_b", "root_a", "from_site", "to_site", "direct", "status", "rounds", "bottleneck", "+inf",
                 "capacity", "rows_out", "NULL", "code 3"):
        assert word in doc, word
    # the cluster block points here instead of saying that the Euclidean gap is not computed
    cl = raw[:raw.index("int dkmc_find_clusters")]
    cl = cl[cl.rindex("/*"):]
    assert "dkmc_find_gaps" in cl and "not computed" not in cl
    # an addition: dkmc_stats keeps its layout
    body = re.sub(r"/\*.*?\*/", "", raw[raw.index("typedef struct dkmc_stats {"):raw.index("} dkmc_stats;")], flags=re.S)
    assert body.strip().rstrip(";").split()[-1] == "x_tile_f32_bytes"


def test_library_exports_and_lib_binds_the_calls():
    import __graft_entry__ as g
    g.build()
    from devicekmc_amd import host, lib
    L = lib.load()
    vp, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    assert lib.SYMBOLS["dkmc_find_gaps"] == (I, [I, vp, vp, vp, vp, I, vp, I, I, D])
    assert lib.SYMBOLS["dkmc_get_gap_info"] == (I, [ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(D)])
    assert lib.SYMBOLS["dkmc_copy_gap_edges"] == (I, [I, vp, vp, vp, vp, vp, ctypes.POINTER(I)])
    assert lib.SYMBOLS["dkmc_copy_gap_chain"] == (I, [I, vp, vp, vp, ctypes.POINTER(I)])
    assert lib.SYMBOLS["dkmc_debug_set_gap_cell_skip"] == (None, [I])
    for n in CALLS + ("dkmc_debug_set_gap_cell_skip",):
        assert hasattr(L, n), n
    assert lib.dkmc_stats._fields_[-1][0] == "x_tile_f32_bytes"
    assert callable(host.find_gaps) and callable(host.Device.find_gaps)


def test_source_keeps_the_contract_arithmetic_unfused():
    """the distance is written with contraction switched off (the fused form differs from numpy's in the last bit)"""
    src = open(os.path.join(ROOT, "devicekmc_amd", "csrc", "gaps.hip")).read()
    body = src[src.index("double gp_d2("):]
    body = body[:body.index("\n}\n")]
    assert "#pragma clang fp contract(off)" in body and "(xx + yy) + zz" in body and "fma(" not in body
