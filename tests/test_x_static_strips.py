"""Host-only arithmetic of dkmc_set_x_static_tiles (csrc/xt_static.h: xs_w_static, through dkmc_x_static_strips): with nM inner-contact metals in
front of S the column strips w < nM / 256 of the tile store hold contact x contact entries only and can be kept; fewer than 256 metals give 0, which
means a full fill.  No GPU needed."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from devicekmc_amd import lib
    return lib.load()


def test_strips_that_can_be_kept(L):
    # 829: the 2.5 nm cell (3 of its 4 strips); 82 900: the benchmark's tile:10 (323 of 363)
    assert [L.dkmc_x_static_strips(n) for n in (0, 255, 256, 829, 82900)] == [0, 0, 1, 3, 323]
    assert L.dkmc_x_static_strips(-5) == 0
    for n in (1, 511, 512, 513, 2 ** 31 - 1):
        w = L.dkmc_x_static_strips(n)
        assert 256 * w <= n < 256 * (w + 1)                  # every column of a kept strip is a metal; the next strip is not all metal or not full


def test_size_rule_of_mode_2(L):
    """7.5nm (8 353 members) and tile:5 (23 224) lose or tie against atom order, tile:6 (33 445) and above gain (profiles/ab_bench_x_static_tiles.txt)."""
    try:
        L.dkmc_debug_set_x_static_gate(0)
        assert [L.dkmc_x_static_rule(n) for n in (-1, 0, 929, 8353, 23224, 32767, 32768, 33445, 92906, 2 ** 31 - 1)] == [0, 0, 0, 0, 0, 0, 1, 1, 1, 1]
        L.dkmc_debug_set_x_static_gate(500)
        assert [L.dkmc_x_static_rule(n) for n in (499, 500, 929)] == [0, 1, 1]
    finally:
        L.dkmc_debug_set_x_static_gate(0)
    assert L.dkmc_x_static_rule(929) == 0


def test_entry_points_are_declared_and_bound_and_default_is_auto(L):
    from devicekmc_amd import lib
    pub = open(os.path.join(ROOT, "include", "devicekmc_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "devicekmc_hip_debug.h")).read()
    for name, src in (("dkmc_set_x_static_tiles", pub), ("dkmc_get_x_static_tiles", pub), ("dkmc_get_x_static_info", pub),
                      ("dkmc_debug_x_static_verify", dbg), ("dkmc_debug_get_x_static_verify", dbg), ("dkmc_x_static_strips", dbg),
                      ("dkmc_xt_get_srow", dbg), ("dkmc_xt_get_diag", dbg), ("dkmc_x_static_rule", dbg),
                      ("dkmc_debug_set_x_static_gate", dbg)):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in lib.SYMBOLS, name
    assert lib.SYMBOLS["dkmc_set_x_static_tiles"] == (None, [ctypes.c_int]) and lib.SYMBOLS["dkmc_get_x_static_tiles"] == (ctypes.c_int, [])
    was = L.dkmc_get_x_static_tiles()
    try:
        assert was == 2
        for mode, got in ((0, 0), (1, 1), (2, 2), (7, 2), (-1, 2)):
            L.dkmc_set_x_static_tiles(mode)
            assert L.dkmc_get_x_static_tiles() == got
    finally:
        L.dkmc_set_x_static_tiles(was)
