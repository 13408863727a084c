"""The size rule of the live view's auto mode (csrc/xt_live.h: xtl_drop_rule, through dkmc_xtl_drop_rule): 1e-10 at and above a gate in stored
sub-blocks, 0.0 below it, with the gate between the largest measured size at which the live view does not gain and the smallest at which it does
(profiles/x_tile_drop_by_size.jsonl: the lines with `gains`).  Host code only, no GPU needed."""
import ctypes
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THETA = 1e-10


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from devicekmc_amd import lib
    return lib.load()


def _measured():
    with open(os.path.join(ROOT, "profiles", "x_tile_drop_by_size.jsonl")) as f:
        recs = [json.loads(line) for line in f if line.strip()]
    return [r for r in recs if "gains" in r]


def test_rule_follows_the_measured_verdict_at_every_measured_size(L):
    got = _measured()
    assert {"7.5nm", "tile:5", "tile:7", "tile:10"} <= set(r["workload"] for r in got)
    assert any(r["gains"] for r in got) and not all(r["gains"] for r in got)
    L.dkmc_set_x_tile_drop_auto_subblocks(0)
    for r in got:
        for d in (-1, 0, 1):
            assert L.dkmc_xtl_drop_rule(int(r["stored_subblocks"]) + d) == (THETA if r["gains"] else 0.0), (r, d)


def test_rule_is_monotone_and_gives_nothing_without_a_size(L):
    L.dkmc_set_x_tile_drop_auto_subblocks(0)
    sizes = sorted(set([1, 2, 3] + [int(10 ** (k / 16.0)) for k in range(0, 16 * 18)] + [2 ** k for k in range(0, 63)] + [2 ** 62] +
                       [int(r["stored_subblocks"]) + d for r in _measured() for d in (-1, 0, 1)]))
    out = [L.dkmc_xtl_drop_rule(n) for n in sizes]
    assert set(out) == {0.0, THETA}, set(out)
    assert all(a <= b for a, b in zip(out, out[1:])), list(zip(sizes, out))
    assert out[0] == 0.0 and out[-1] == THETA
    assert [L.dkmc_xtl_drop_rule(n) for n in (0, -1, -2 ** 62)] == [0.0, 0.0, 0.0]


def test_gate_can_be_moved_and_restored(L):
    try:
        L.dkmc_set_x_tile_drop_auto_subblocks(0)
        sizes = (1, 99, 100, 101, 10 ** 9)
        before = [L.dkmc_xtl_drop_rule(n) for n in sizes]
        assert before[:4] == [0.0] * 4 and before[4] == THETA
        L.dkmc_set_x_tile_drop_auto_subblocks(100)
        assert [L.dkmc_xtl_drop_rule(n) for n in sizes] == [0.0, 0.0, THETA, THETA, THETA]
        L.dkmc_set_x_tile_drop_auto_subblocks(1)
        assert [L.dkmc_xtl_drop_rule(n) for n in (0, 1, 2)] == [0.0, THETA, THETA]
    finally:
        L.dkmc_set_x_tile_drop_auto_subblocks(0)
    assert [L.dkmc_xtl_drop_rule(n) for n in sizes] == before
    L.dkmc_set_x_tile_drop_auto_subblocks(-5)                              # anything below 1: the measured gate
    assert [L.dkmc_xtl_drop_rule(n) for n in sizes] == before


def test_entry_points_are_declared_and_bound(L):
    from devicekmc_amd import lib
    pub = open(os.path.join(ROOT, "include", "devicekmc_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "devicekmc_hip_debug.h")).read()
    want = {"dkmc_set_x_tile_drop_auto": (pub, (None, [ctypes.c_int])), "dkmc_get_x_tile_drop_auto": (pub, (ctypes.c_int, [])),
            "dkmc_get_x_tile_drop_used": (pub, (ctypes.c_double, [])), "dkmc_xtl_drop_rule": (dbg, (ctypes.c_double, [ctypes.c_longlong])),
            "dkmc_set_x_tile_drop_auto_subblocks": (dbg, (None, [ctypes.c_longlong]))}
    for name, (src, sig) in want.items():
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert lib.SYMBOLS.get(name) == sig, name
    for name in ("dkmc_xtl_drop_rule", "dkmc_set_x_tile_drop_auto_subblocks"):
        assert not re.search(r"\b%s\s*\(" % name, pub), name               # test aids stay out of the public header
    # the counts of the live view reuse existing fields: no offset of dkmc_stats moved
    assert lib.dkmc_stats.xt_local_subblocks.offset == lib.dkmc_stats.xt_subblocks.offset + 8
    assert lib.dkmc_stats.xb_poly_used.offset == lib.dkmc_stats.xb_aux.offset + 4 == lib.dkmc_stats.xb_width.offset - 4


def test_fresh_library_defaults(L):
    assert L.dkmc_get_x_tile_drop() == 0.0
    assert L.dkmc_get_x_tile_drop_auto() == 1
    assert L.dkmc_get_x_tile_drop_used() == 0.0
