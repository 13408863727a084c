"""The plain reference of the event loop (tests/event_loop_ref.py) is pinned to the CPU oracle's okmc_execute_events on tables with exact sums
before tests/test_gpu_event_loop.py trusts it, and to hand-made cases where the oracle has no answer (a draw of 1.0, a table that runs dry);
the test aid dkmc_debug_event_loop is declared, bound and exported.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import event_loop_cases as cases
import event_loop_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle_run(c, seed, max_events, freq):
    """okmc_execute_events on the case's table (as doubles: k 2^s SCALE, every prefix exact) with draws from OracleRNG(seed)."""
    from oracle import oracle as oc
    L = oc.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    neigh = np.ascontiguousarray(c.neigh, dtype=np.int32)
    ev_type = ref.slot_classes(neigh, c.element); ev_prob = c.table.astype(np.float64) * cases.SCALE
    el, q = c.element.copy(), c.charge.copy()
    log = np.zeros((max_events, 4), dtype=np.int32); margin = np.zeros(max_events); psum = np.zeros(max_events)
    et = C.c_double(0)
    n = L.okmc_execute_events(c.N, c.nn, p(neigh), p(ev_type), p(ev_prob), C.c_double(freq), p(el), p(q), oc.OracleRNG(seed).buf, max_events,
                              p(log), p(margin), p(psum), C.byref(et))
    return dict(n=n, log=log[:n], margin=margin[:n], psum=psum[:n], dt=et.value, element=el, charge=q)


@pytest.mark.parametrize("shape", [(5, 1), (63, 3), (64, 64), (65, 65), (257, 130), (4097, 2)])
@pytest.mark.parametrize("stop", ["time", "draws", "dry"])
def test_reference_is_the_oracle_loop(shape, stop):
    from oracle import oracle as oc
    N, nn = shape
    c = cases.build_case(N, nn, 1, p_edge=0.3)
    Psum0 = float(c.table.sum()) * cases.SCALE
    # time: the waiting times end the step after a few events; draws: after max_events; dry: neither does, the table runs out
    freq, max_events = {"time": (Psum0 / 6, 500), "draws": (Psum0 * 2.0 ** -70, 3), "dry": (Psum0 * 2.0 ** -70, 3000)}[stop]
    seed = 77 + N
    o = _oracle_run(c, seed, max_events, freq)
    rng = oc.OracleRNG(seed)
    draws = [rng.uniform() for _ in range(2 * max_events)]
    r = ref.run(c.table, c.neigh, c.element, c.charge, freq, draws, cases.SCALE)
    print(shape, stop, "events", r["n_events"], "exhausted", r["exhausted"], "dry", r["dry"])
    assert r["n_events"] == o["n"] and np.array_equal(r["log"], o["log"])
    assert np.array_equal(r["element"], o["element"]) and np.array_equal(r["charge"], o["charge"])
    assert r["dt"] == o["dt"]                                           # the same double operations on the same exact Psum; inf when dry
    assert np.array_equal(r["margin"] / (np.array(r["loop"].psums) / cases.SCALE), o["margin"])
    if stop == "draws" and N > 5:
        assert r["exhausted"] and not r["dry"] and r["n_events"] == 3
    if stop == "dry":
        assert r["dry"] and not r["exhausted"] and r["dt"] == float("inf") and not (r["loop"].P > 0).any()
    if stop == "time" and N > 5:
        assert not r["dry"] and not r["exhausted"] and r["n_events"] >= 2 and not r["dt"] < 1 / freq


def _tiny():
    """Four sites in a path 0 - 1 - 2 - 3, nn = 2; rates 3, 0 | 5, 8 | 2, 0 | 6, 0 in row order; prefixes 3 3 8 16 18 18 24 24."""
    neigh = np.array([1, -1, 2, 0, 3, 1, 2, -1], dtype=np.int32)
    table = np.array([3, 0, 5, 8, 2, 0, 6, 0], dtype=np.int64)
    element = np.array([ref.DEFECT, ref.O_EL, ref.VACANCY, ref.OXYGEN_DEFECT], dtype=np.int32)
    charge = np.array([0, 0, 2, -2], dtype=np.int32)
    return neigh, table, element, charge


def test_hand_made_draws():
    neigh, table, element, charge = _tiny()
    cases.check_index(neigh, 4, 2)
    assert list(np.cumsum(table)) == [3, 3, 8, 16, 18, 18, 24, 24]
    pick = lambda u: ref.EventLoop(table, neigh, element, charge, 1.0).select(u)
    assert pick(0.0) == (0, 0.0)                                        # a draw of 0: the first positive slot
    assert pick(0.125) == (2, 0.0)                                      # number == 3, an edge: the prefix 3 does not EXCEED it, slots 0 and 1 are passed
    assert pick(np.nextafter(0.125, 0.0))[0] == 0                       # one ulp below that edge
    assert pick(8 / 24) == (3, 0.0) and 8 / 24 * 24.0 == 8.0
    assert pick(0.75) == (6, 0.0)                                       # number == 18: over the zero slot 5 to the next positive one
    assert pick(1.0 - 2.0 ** -53)[0] == 6
    assert pick(1.0) == (6, 0.0)                                        # a draw of 1.0: no prefix exceeds 24, the LAST positive slot
    # the classes, from the elements at execution time
    lp = ref.EventLoop(table, neigh, element, charge, 1.0)
    dt = lp.step(0.0, np.exp(-1.0))                                     # slot 0: (DEFECT, O) generation
    assert lp.log == [(0, 0, 1, ref.EV_GEN)] and dt == -np.log(np.exp(-1.0)) / 24.0
    assert list(lp.element) == [ref.OXYGEN_DEFECT, ref.VACANCY, ref.VACANCY, ref.OXYGEN_DEFECT] and list(lp.charge) == [-2, 2, 2, -2]
    assert list(lp.P) == [0, 0, 0, 0, 2, 0, 6, 0]                       # rows 0, 1 and the slot of row 2 that targets 1
    lp.step(0.5, 0.5)                                                   # slot 6: (Od, V) recombination
    assert lp.log[1] == (6, 3, 2, ref.EV_REC) and list(lp.element) == [ref.OXYGEN_DEFECT, ref.VACANCY, ref.O_EL, ref.DEFECT]
    assert list(lp.charge) == [-2, 2, 0, 0] and lp.psum == 0 and lp.step(0.5, 0.5) is None
    # no class: type EV_NULL, nothing moves, the slots are zeroed all the same
    el = np.array([4, 4, 0, 0], dtype=np.int32)
    lp = ref.EventLoop(table, neigh, el, charge, 1.0)
    lp.step(0.0, 0.5)
    assert lp.log == [(0, 0, 1, ref.EV_NULL)] and list(lp.element) == list(el) and list(lp.charge) == list(charge) and lp.psum == 8
    # the diffusion classes swap elements and charges
    for a, b, cls in ((ref.VACANCY, ref.O_EL, ref.EV_VDIFF), (ref.OXYGEN_DEFECT, ref.DEFECT, ref.EV_IDIFF)):
        lp = ref.EventLoop(table, neigh, np.array([a, b, 4, 4], dtype=np.int32), np.array([1, -1, 0, 0], dtype=np.int32), 1.0)
        lp.step(0.0, 0.5)
        assert lp.log == [(0, 0, 1, cls)] and list(lp.element[:2]) == [b, a] and list(lp.charge[:2]) == [-1, 1]


def test_hand_made_stops():
    neigh, table, element, charge = _tiny()
    freq = 1.0
    small, big = float(np.exp(-24.0 * 0.25)), float(np.exp(-24.0 * 4.0))           # dt = 1 / 4 and 4 on the full table
    # runs dry: two events, then no positive rate
    r = ref.run(table, neigh, element, charge, freq, [0.0, small, 0.5, 1.0, 0.5, 0.5])
    assert r["n_events"] == 2 and r["dry"] and not r["exhausted"] and r["dt"] == float("inf")
    # the waiting time stops it: !(dt < 1 / freq), at equality too
    r = ref.run(table, neigh, element, charge, freq, [0.0, big, 0.5, 0.5])
    assert r["n_events"] == 1 and not r["dry"] and not r["exhausted"] and r["dt"] == -np.log(big) / 24.0 >= 2.0
    # the draws run out: 2 n + 1 >= n_uniform before each selection
    for n_uniform, want in ((0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (5, 2)):
        r = ref.run(table, neigh, element, charge, freq, [0.0, small, 0.5, 1.0, 0.5][:n_uniform])
        assert (r["n_events"], r["exhausted"], r["dry"]) == (want, True, False), n_uniform
    # a resumed loop goes on where the first call stopped, its log is its own
    r1 = ref.run(table, neigh, element, charge, freq, [0.0, small, 0.9])
    r2 = ref.run(None, None, None, None, None, [0.5, 1.0, 0.5, 0.5], loop=r1["loop"])
    assert r1["n_events"] == 1 and r1["exhausted"] and r2["n_events"] == 1 and r2["dry"] and r2["log"].tolist() == [[6, 3, 2, ref.EV_REC]]
    # a table in np.longdouble: the same picks, margins in table units
    r = ref.run(table.astype(np.longdouble), neigh, element, charge, freq, [0.26, small, 0.5, 1.0, 0.5, 0.5])
    assert r["log"][0].tolist() == [2, 1, 2, ref.EV_NULL] and abs(r["margin"][0] - 1.76) < 1e-12


def test_case_recipe_conditions():
    """The recipe of the GPU test on one small shape: edges hit exactly, the fallback draw present, waiting times well away from the stop."""
    c = cases.build_case(65, 65, 1, p_edge=0.9, weights=(0.75, 0.1, 0.03, 0.02, 0.1))
    assert c.kinds[1] == "one" and c.n_edge >= 10 and c.ref["n_events"] == len(c.kinds) >= 15
    on_edge = (c.ref["margin"] == 0) & (np.array(c.kinds) == "edge")
    assert on_edge.sum() == c.n_edge
    again = cases.build_case.__wrapped__(65, 65, 1, p_edge=0.9, weights=(0.75, 0.1, 0.03, 0.02, 0.1))
    assert again.draws.tobytes() == c.draws.tobytes() and np.array_equal(again.ref["log"], c.ref["log"])


def _header(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", " ", src, flags=re.S)


def test_header_declares_the_aid():
    pub, dbg = _header("devicekmc_hip.h"), _header("devicekmc_hip_debug.h")
    m = re.search(r"\bint\s+dkmc_debug_event_loop\s*\(([^)]*)\)\s*;", dbg)
    assert m and "dkmc_debug_event_loop" not in pub
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 14
    assert re.fullmatch(r"const\s+int\s*\*\s*d_neigh_idx", args[2]) and re.fullmatch(r"const\s+double\s*\*\s*d_ev_prob_in", args[3])
    assert re.fullmatch(r"const\s+double\s*\*\s*h_uniform", args[7]) and args[8:10] == ["int n_uniform", "int resume"]
    assert re.fullmatch(r"double\s*\*\s*event_time_out", args[13])
    raw = open(os.path.join(ROOT, "include", "devicekmc_hip_debug.h")).read()
    doc = raw[raw.index("Test aid of the event loop"):raw.index("int dkmc_debug_event_loop(")]
    for word in ("[-1, N)", "symmetric", "finite values >= 0", "discards a pending resume", "error 7", "out of bounds"):
        assert word in doc, word


def test_library_exports_and_lib_binds_the_aid():
    import __graft_entry__ as g
    g.build()
    from devicekmc_amd import lib
    L = lib.load()
    vp, I = C.c_void_p, C.c_int
    assert lib.SYMBOLS["dkmc_debug_event_loop"] == (I, [I, I, vp, vp, vp, vp, vp, vp, I, I, C.POINTER(I), C.POINTER(I), vp, C.POINTER(C.c_double)])
    assert hasattr(L, "dkmc_debug_event_loop")
    # bad arguments are refused before anything touches a device
    n, ex, et = C.c_int(-1), C.c_int(-1), C.c_double(-1.0)
    assert L.dkmc_debug_event_loop(0, 2, None, None, None, None, None, None, 0, 0, C.byref(n), C.byref(ex), None, C.byref(et)) == 13
    assert b"debug_event_loop" in L.dkmc_last_error() and n.value == -1
    L.dkmc_clear_error()
