"""The rule that gives the one-GPU preconditioned block-CG its degree from the rows of the system (csrc/xtb_precond.h: xtb_poly_rule, through
dkmc_xtb_poly_rule): a monotone step function inside 1 ... 16 that returns, at every size the degree series was measured at, the degree recorded as
best there (profiles/x_poly_degree_by_size.jsonl: the lines with `best_degree`).  Host code only, no GPU needed."""
import ctypes
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XB_MAXPOLY = 16


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from devicekmc_amd import lib
    return lib.load()


def _measured():
    with open(os.path.join(ROOT, "profiles", "x_poly_degree_by_size.jsonl")) as f:
        recs = [json.loads(line) for line in f if line.strip()]
    return [r for r in recs if "best_degree" in r]


def test_rule_returns_the_best_measured_degree_at_every_measured_size(L):
    best = _measured()
    assert {"7.5nm", "tile:3", "tile:5", "tile:10"} <= set(r["workload"] for r in best)
    L.dkmc_set_x_poly_auto_rows(0, 0)
    for r in best:
        assert L.dkmc_xtb_poly_rule(int(r["rows"])) == int(r["best_degree"]), r


def test_rule_is_a_monotone_step_function_within_the_degrees_the_solver_has(L):
    L.dkmc_set_x_poly_auto_rows(0, 0)
    sizes = sorted(set([3, 4, 5] + [int(10 ** (k / 16.0)) for k in range(16, 16 * 8)] + [r["rows"] + d for r in _measured() for d in (-1, 0, 1)] + [2 ** 31 - 1]))
    degrees = [L.dkmc_xtb_poly_rule(m) for m in sizes]
    assert all(1 <= d <= XB_MAXPOLY for d in degrees), degrees
    assert all(a <= b for a, b in zip(degrees, degrees[1:])), list(zip(sizes, degrees))
    assert len(set(degrees)) <= 3
    assert [L.dkmc_xtb_poly_rule(m) for m in (-1, 0, 1, 2)] == [0, 0, 0, 0]          # no system: no preconditioner, as in the solver


def test_breakpoints_can_be_moved_and_restored(L):
    try:
        first, last = L.dkmc_xtb_poly_rule(3), L.dkmc_xtb_poly_rule(2 ** 31 - 1)
        L.dkmc_set_x_poly_auto_rows(100, 200)
        got = [L.dkmc_xtb_poly_rule(m) for m in (3, 99, 100, 199, 200, 10 ** 6)]
        assert got[0] == got[1] == first and got[2] == got[3] and got[4] == got[5] == last and first <= got[2] <= last, got
    finally:
        L.dkmc_set_x_poly_auto_rows(0, 0)
    assert L.dkmc_xtb_poly_rule(3) == first and L.dkmc_xtb_poly_rule(2 ** 31 - 1) == last


def test_entry_points_are_declared_and_bound_and_the_stats_carry_the_degree():
    from devicekmc_amd import lib
    pub = open(os.path.join(ROOT, "include", "devicekmc_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "devicekmc_hip_debug.h")).read()
    for name, src in (("dkmc_set_x_poly_auto", pub), ("dkmc_get_x_poly_auto", pub), ("dkmc_set_x_poly_auto_rows", dbg), ("dkmc_xtb_poly_rule", dbg)):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in lib.SYMBOLS, name
    assert lib.SYMBOLS["dkmc_set_x_poly_auto"] == (None, [ctypes.c_int]) and lib.SYMBOLS["dkmc_get_x_poly_auto"] == (ctypes.c_int, [])
    # the degree of the last solve sits in the int beside xb_aux (a padding word before): no offset of dkmc_stats moved
    assert lib.dkmc_stats.xb_poly_used.offset == lib.dkmc_stats.xb_aux.offset + 4 == lib.dkmc_stats.xb_width.offset - 4
    assert re.search(r"\bxb_poly_used\b", pub)
