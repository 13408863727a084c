"""dkmc_set_x_tile_f32 and its aids: declared in the headers, bound in lib.py, and the two stats fields appended at the END of dkmc_stats (existing
offsets do not move).  No GPU: nothing is loaded."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_entry_points_are_declared_and_bound():
    from devicekmc_amd import lib
    pub, dbg = _header("devicekmc_hip.h"), _header("devicekmc_hip_debug.h")
    for name, src in (("dkmc_set_x_tile_f32", pub), ("dkmc_get_x_tile_f32", pub), ("dkmc_debug_fail_true_residual_once", dbg),
                      ("dkmc_xtb_tile_product", dbg), ("dkmc_xt_get_tiles", dbg), ("dkmc_xtb_time_apply_stored", dbg)):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in lib.SYMBOLS, name
    assert lib.SYMBOLS["dkmc_set_x_tile_f32"] == (None, [ctypes.c_int]) and lib.SYMBOLS["dkmc_get_x_tile_f32"] == (ctypes.c_int, [])


def test_stats_layout_matches_header_and_new_fields_are_last():
    from devicekmc_amd import lib
    src = _header("devicekmc_hip.h")
    body = re.sub(r"/\*.*?\*/", "", src[src.index("typedef struct dkmc_stats {"):src.index("} dkmc_stats;")], flags=re.S)
    fields = []
    for line in body.splitlines()[1:]:
        line = line.strip().rstrip(";")
        if not line:
            continue
        typ, rest = re.match(r"(long long|int|double)\s+(.*)$", line).groups()
        for f in rest.split(","):
            fields.append((typ.strip(), f.strip()))
    ctype = {"int": ctypes.c_int, "double": ctypes.c_double, "long long": ctypes.c_longlong}
    assert [(f, ctype[t]) for t, f in fields] == [(f[0], f[1]) for f in lib.dkmc_stats._fields_]
    assert [f for _, f in fields][-3:] == ["x_tile_stream", "x_tile_f64_rounds", "x_tile_f32_bytes"]
    # appended: everything up to xb_fallback keeps its offset (the struct up to there was a multiple of 8 bytes, so no padding moved in)
    assert lib.dkmc_stats.x_tile_stream.offset == lib.dkmc_stats.xb_fallback.offset + 4
    assert lib.dkmc_stats.x_tile_f32_bytes.offset == lib.dkmc_stats.x_tile_stream.offset + 8
    assert ctypes.sizeof(lib.dkmc_stats) == lib.dkmc_stats.x_tile_f32_bytes.offset + 8
