"""The numpy restatement of the event table (tests/event_temp_ref.py) is pinned to the CPU oracle in mode 0 before the GPU tests trust its modes
1 and 2; the two bitwise identities of the rate models hold for the restatement itself; the new parameters and exports exist.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import event_temp_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Vd = 5.0


def _oracle(cell, seed=None):
    from devicekmc_amd import params as pm
    from oracle import oracle as oc
    p = pm.KMCParameters()
    o = oc.OracleKMC(cell.element, cell.x, cell.y, cell.z, p)
    if seed is None:
        o.set_laplace_potential(Vd); o.update_charge(); o.update_potential(Vd)
    else:
        el, pb, pc = er.randomised_state(seed, o.element, o.x)
        o.element[:] = el; o.update_charge()
        o.pot_boundary[:] = pb; o.pot_charge[:] = pc
    return o


@pytest.fixture(scope="module")
def states(cell_2p5):
    return {s: _oracle(cell_2p5, s) for s in (None, 11, 12, 13)}


@pytest.mark.parametrize("seed", [None, 11, 12, 13])
def test_mode0_is_the_oracle_table(states, seed):
    o = states[seed]
    ot, op = o.build_event_list()
    t, P, n_bad = er.oracle_tables(o, 0)
    assert n_bad == 0 and np.array_equal(t, ot)
    assert np.array_equal(P > 0, op > 0) and np.array_equal(np.isfinite(P), np.isfinite(op))
    m = (op > 0) & np.isfinite(op)
    assert m.sum() > 0
    assert np.abs(P[m] / op[m] - 1).max() <= 1e-12
    if seed is not None:
        for c in range(4):
            assert (ot == c).sum() > 0, c


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_bitwise_identities_of_the_restatement(states, seed):
    o = states[seed]
    _, P0, _ = er.oracle_tables(o, 0)
    uniform = np.full(o.N, o.T_bg)
    ball = er.ball_field(o.x, o.y, o.z, o.T_bg)
    assert (ball > o.T_bg).sum() > 10 and (ball == o.T_bg).sum() > o.N // 2 and ball.max() <= o.T_bg + 300.0
    T_s, cls = er.deciding_temperature(o.neigh, o.element, ball)
    cold = T_s == o.T_bg
    for mode in (1, 2):
        t, P, n_bad = er.oracle_tables(o, mode, uniform)
        assert n_bad == 0 and np.array_equal(P, P0)                       # (a): T_s == T_bg everywhere gives mode 0's bits
        t, P, n_bad = er.oracle_tables(o, mode, ball)
        assert n_bad == 0 and np.array_equal(P[cold], P0[cold])           # (b): ... and slot by slot under any field
        hot = (cls != er.EV_NULL) & ~cold & (P0 > 0) & np.isfinite(P0)
        assert hot.sum() > 0 and (P[hot] != P0[hot]).sum() >= 900 // 2     # the hot slots do move
    # bad temperatures: counted, zero rate, type kept
    bad = ball.copy()
    rows = np.unique(np.flatnonzero((cls != er.EV_NULL) & (cls != er.EV_GEN)) // o.nn)[:3]
    bad[rows[0]], bad[rows[1]], bad[rows[2]] = np.nan, 0.0, -5.0
    t, P, n_bad = er.oracle_tables(o, 2, bad)
    Tb, _ = er.deciding_temperature(o.neigh, o.element, bad)
    want = (cls != er.EV_NULL) & ~(np.isfinite(Tb) & (Tb > 0))
    assert n_bad == want.sum() >= 3 and (P[want] == 0).all() and np.array_equal(t, er.oracle_tables(o, 0)[0])


def test_census_of_the_restatement(states):
    o = states[11]
    ball = er.ball_field(o.x, o.y, o.z, o.T_bg)
    t, P, _ = er.oracle_tables(o, 2, ball)
    P = P.copy(); P[5] = np.inf; P[77] = np.nan
    info = er.census(o.neigh, o.element, P, ball)
    live = np.isfinite(P) & (P > 0)
    assert info[14] == 2 and info[15] == live.sum() == info[:4].sum()
    for c in range(4):
        assert info[c] == (live & (t == c)).sum()
        assert o.T_bg * (1 - 1e-12) <= info[8 + c] / info[4 + c] <= (o.T_bg + 300.0) * (1 + 1e-12)      # a weighted mean of the field, to rounding
    assert info[12] == P[live].max() and P[int(info[13])] == info[12]
    none = er.census(o.neigh, o.element, P)
    assert (none[8:12] == 0).all() and np.array_equal(np.delete(none, range(8, 12)), np.delete(info, range(8, 12)))
    empty = er.census(o.neigh, o.element, np.zeros_like(P), ball)
    assert (empty[:13] == 0).all() and empty[13] == -1 and empty[14] == 0 and empty[15] == 0


def test_parameters():
    import copy
    from devicekmc_amd import params as pm
    p = pm.KMCParameters()
    assert p.event_temperature == 0 and p.event_census is False
    q = pm.KMCParameters(event_temperature=2, event_census=True)
    assert (q.event_temperature, q.event_census) == (2, True)
    assert copy.deepcopy(q).for_tiling(2).event_temperature == 2 and q.log_revision().event_census is True


def _header(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", " ", src, flags=re.S)


def test_headers_declare_the_calls():
    pub, dbg = _header("devicekmc_hip.h"), _header("devicekmc_hip_debug.h")
    assert re.search(r"\bvoid\s+dkmc_set_event_temperature\s*\(\s*int\s+\w+\s*\)\s*;", pub)
    assert re.search(r"\bint\s+dkmc_get_event_temperature\s*\(\s*void\s*\)\s*;", pub)
    m = re.search(r"\bint\s+dkmc_build_event_list_T\s*\(([^)]*)\)\s*;", pub)
    assert m and len(m.group(1).split(",")) == 21 and re.search(r"const\s+double\s*\*\s*d_site_temperature\s*,\s*int\s*\*\s*d_n_bad\s*$", m.group(1).strip())
    m0 = re.search(r"\bint\s+dkmc_build_event_list\s*\(([^)]*)\)\s*;", pub)
    assert m0 and len(m0.group(1).split(",")) == 19                                  # keeps its signature
    m = re.search(r"\bint\s+dkmc_event_rate_census\s*\(([^)]*)\)\s*;", pub)
    assert m and len(m.group(1).split(",")) == 7 and re.search(r"double\s*\*\s*h_info16\s*$", m.group(1).strip())
    assert re.search(r"\bvoid\s+dkmc_set_event_census\s*\(\s*int\s+\w+\s*\)\s*;", pub)
    assert re.search(r"\bint\s+dkmc_get_event_census\s*\(\s*double\s*\*\s*\w+\s*\)\s*;", pub)
    assert re.search(r"\bint\s+dkmc_debug_get_event_times\s*\(\s*double\s*\*\s*\w+\s*\)\s*;", dbg) and "debug_get_event_times" not in pub
    raw = open(os.path.join(ROOT, "include", "devicekmc_hip.h")).read()
    doc = raw[raw.index("event rates on the local site temperature"):raw.index("int dkmc_get_event_census(")]
    for word in ("deciding site", "GENERATION", "kinetic", "Arrhenius", "not finite or not > 0", "local heat model", "info16", "rate-weighted",
                 "non-finite", "bit for bit"):
        assert word in doc, word
    # an addition: dkmc_stats keeps its layout
    body = re.sub(r"/\*.*?\*/", "", raw[raw.index("typedef struct dkmc_stats {"):raw.index("} dkmc_stats;")], flags=re.S)
    assert body.strip().rstrip(";").split()[-1] == "x_tile_f32_bytes"
    shim = open(os.path.join(ROOT, "include", "gpu_solvers.h")).read()
    assert re.search(r"void\s+set_event_temperature\s*\(\s*const\s+int\s+mode\s*\)", shim) and re.search(r"void\s+event_rate_census\s*\(", shim)


def test_library_exports_and_lib_binds_the_calls():
    import __graft_entry__ as g
    g.build()
    from devicekmc_amd import host, lib
    L = lib.load()
    vp, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double)
    assert lib.SYMBOLS["dkmc_set_event_temperature"] == (None, [I]) and lib.SYMBOLS["dkmc_get_event_temperature"] == (I, [])
    assert lib.SYMBOLS["dkmc_build_event_list_T"] == (I, [I, I, vp, vp, vp, I] + [vp] * 15)
    assert lib.SYMBOLS["dkmc_event_rate_census"] == (I, [I, I, vp, vp, vp, vp, D])
    assert lib.SYMBOLS["dkmc_set_event_census"] == (None, [I]) and lib.SYMBOLS["dkmc_get_event_census"] == (I, [D])
    for n in ("dkmc_set_event_temperature", "dkmc_get_event_temperature", "dkmc_build_event_list_T", "dkmc_event_rate_census",
              "dkmc_set_event_census", "dkmc_get_event_census_on", "dkmc_get_event_census", "dkmc_debug_get_event_times"):
        assert hasattr(L, n), n
    assert lib.dkmc_stats._fields_[-1][0] == "x_tile_f32_bytes"
    # the switches are plain engine state: no device is touched
    try:
        assert L.dkmc_get_event_temperature() == 0 and L.dkmc_get_event_census_on() == 0
        for mode, want in ((1, 1), (2, 2), (3, 0), (-1, 0), (0, 0)):
            L.dkmc_set_event_temperature(mode)
            assert L.dkmc_get_event_temperature() == want
        L.dkmc_set_event_census(5)
        assert L.dkmc_get_event_census_on() == 1
    finally:
        L.dkmc_set_event_temperature(0); L.dkmc_set_event_census(0)
    # no step has taken a census in a process without a GPU: the getter fails with its own code and says why
    rc = L.dkmc_get_event_census((ctypes.c_double * 16)())
    if rc != 0:
        assert rc == 17 and b"no census" in L.dkmc_last_error()
        L.dkmc_clear_error()
    assert callable(host.event_rate_census) and host.EVENT_CLASSES == ("gen", "rec", "vdiff", "idiff")


def test_steplog_census_keys():
    from devicekmc_amd import io as kio
    from devicekmc_amd import host
    res = {"Current [uA]": 11.8834}
    a, b = kio.StepLog(), kio.StepLog()
    a.step(0, 5, 2e-14, res); b.step(0, 5, 2e-14, res, census=None)
    assert a.text() == b.text() and "Event rate" not in a.text()
    c = kio.StepLog()
    c.step(0, 5, 2e-14, res, census=host._census_dict([3, 1, 2, 0, 6.0, 1.0, 1.0, 0.0, 1800.0, 300.0, 300.0, 0.0, 4.0, 17, 0, 6]))
    lines = c.text().splitlines()
    assert "Event rate total [1/s]: 8" in lines and "Event rate share gen/rec/vdiff/idiff: 0.75/0.125/0.125/0" in lines
    assert lines.index("Current [uA]: 11.8834") < lines.index("Event rate share gen/rec/vdiff/idiff: 0.75/0.125/0.125/0") < lines.index("Event rate total [1/s]: 8")
