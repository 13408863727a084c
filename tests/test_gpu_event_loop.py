"""The event loop of a KMC step (csrc/events.hip: k_ev_loop -- tree descent, execution, zeroing, tree repair, waiting time, stop) against its
sequential definition tests/event_loop_ref.py (pinned to the CPU oracle by tests/test_event_loop_ref.py).

Exact layer: through the test aid dkmc_debug_event_loop the PRODUCTION loop runs on tables of rates k 2^s whose grand total stays below 2^52 units:
every partial sum is exact in every order, so the device must pick the reference's slot for EVERY draw -- on a bucket edge, one ulp below it, 0,
1 - 2^-53 and 1.0 included; nothing is exempt.  Shapes are the smallest at which each path of the tree exists (one group, 64 k and 64 k + 1 rows,
4096 k and 4096 k + 1, a second chunk of the top level at 262 145 rows, rows longer than one wave).  Every event retires two sites, so a shape of N
sites has at most N / 2 events; the tiny and the dense shapes run dry (error 7) before the 70 events a case asks for, and take more than one seed
to collect the 20 events on an edge that every shape must show.

Production layer: dkmc_execute_kmc_step_gpu on synthetic physical states gives the aid's log bit for bit on the table read back from
dkmc_build_event_list_T, and the reference's on that table in np.longdouble; the seeds are chosen so that no draw lies within 1e-9 Psum of an edge."""
import copy
import ctypes as C

import numpy as np
import pytest

import event_loop_cases as cases
import event_loop_ref as ref

pytestmark = pytest.mark.gpu

Vd = 5.0
W_DENSE = (0.75, 0.1, 0.03, 0.02, 0.1)          # shapes that run dry after a few dozen events draw on edges three times out of four

# shape -> (seeds, recipe, events of the reference over these seeds).  (2, 1) and (5, 1) hold one and at most two events per table; every eighth
# seed opens with the draw of 1.0.
SHAPES = {
    (2, 1): (range(80), dict(weights=W_DENSE, p_edge=1.0), 80),
    (5, 1): (range(30), dict(weights=W_DENSE, p_edge=1.0), 50),
    (63, 3): (range(2), dict(weights=W_DENSE, p_edge=0.2), 53),
    (64, 64): (range(2), dict(weights=W_DENSE, p_edge=0.7), 64),
    (65, 65): (range(2), dict(weights=W_DENSE, p_edge=0.9), 64),
    (257, 130): (range(1), dict(p_edge=0.6), 70),
    (4096, 2): (range(1), {}, 70),
    (4097, 2): (range(1), {}, 70),
    (262145, 2): (range(1), {}, 70),
}


def case(N, nn, seed):
    kw = dict(SHAPES[(N, nn)][1])
    if N <= 5:
        kw["one_at"] = 0 if seed % 8 == 7 else -1
    return cases.build_case(N, nn, seed, **kw)


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__ as g
    g.build()
    from devicekmc_amd import host, lib
    assert _torch().cuda.is_available()
    return host, lib.load()


def _dev(a, dtype=None):
    return _torch().as_tensor(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


class OnDevice:
    """The index, table, state and freq of a case on the device; reset() puts the state before any event back."""

    def __init__(self, c):
        cases.check_index(c.neigh, c.N, c.nn)                           # the loop trusts its index: entries in [-1, N), symmetric
        self.c = c
        self.neigh = _dev(c.neigh, np.int32)
        self.table = _dev(c.table.astype(np.float64) * cases.SCALE)
        self.freq = _dev(np.array([c.freq]))
        self.reset()

    def reset(self):
        self.element, self.charge = _dev(self.c.element, np.int32), _dev(self.c.charge, np.int32)

    def state(self):
        return self.element.cpu().numpy(), self.charge.cpu().numpy()


def aid(hip, d, N, nn, draws, resume):
    """One call of dkmc_debug_event_loop: (rc, n_events, exhausted, log, event_time).  Error 7 is part of the interface: checked and cleared."""
    host, L = hip
    from devicekmc_amd.host import _ptr
    host._use_stream("cuda:0")
    draws = np.ascontiguousarray(draws, dtype=np.float64)
    log = np.full((max(len(draws) // 2, 1), 4), -9, dtype=np.int32)
    n, ex, et = C.c_int(-1), C.c_int(-1), C.c_double(-1.0)
    rc = L.dkmc_debug_event_loop(N, nn, _ptr(d.neigh), _ptr(d.table), _ptr(d.element), _ptr(d.charge), _ptr(d.freq),
                                 draws.ctypes.data_as(C.c_void_p), len(draws), resume, C.byref(n), C.byref(ex), log.ctypes.data_as(C.c_void_p), C.byref(et))
    if rc != 0:
        msg = L.dkmc_last_error()
        L.dkmc_clear_error()
        assert rc == 7 and b"no event with a positive rate" in msg, (rc, msg)
    assert (log[n.value:] == -9).all()
    return rc, n.value, ex.value, log[:n.value], et.value


def batched(hip, d, c, n_uniform):
    """The case's draws handed over n_uniform at a time, as the host does it: two draws consumed per event, resume after the first call."""
    pos, resume, logs, calls = 0, 0, [], 0
    while True:
        rc, n, ex, log, et = aid(hip, d, c.N, c.nn, c.draws[pos:pos + n_uniform], resume)
        logs.append(log); pos += 2 * n; resume = 1; calls += 1
        if rc or not ex:
            return rc, np.concatenate(logs), ex, et, calls
        assert n == n_uniform // 2 and len(c.draws) - pos >= 2


def check_against_reference(c, rc, log, ex, et, element, charge):
    r = c.ref
    assert len(log) == r["n_events"]
    bad = np.flatnonzero((log != r["log"]).any(axis=1))
    assert len(bad) == 0, "event %d (draw kind %s): device %s, reference %s" % (bad[0], c.kinds[bad[0]], log[bad[0]], r["log"][bad[0]])
    assert rc == (7 if r["dry"] else 0) and ex == 0
    if r["dry"]:
        assert et == float("inf")
    else:
        assert abs(et / r["dt"] - 1) <= 1e-12                           # the figure of test_default_tolerance_superstep_7p5
    assert np.array_equal(element, r["element"]) and np.array_equal(charge, r["charge"])


# ---- 1. exact layer ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_exact_tables(hip, shape):
    N, nn = shape
    seeds, _, want_events = SHAPES[shape]
    n_edge = n_events = n_one = g64 = g4096 = chunk = high = 0
    for seed in seeds:
        c = case(N, nn, seed)
        r, lg = c.ref, c.ref["log"]
        # what the inputs were chosen for, on the reference alone
        on_edge = (np.array(c.kinds) == "edge")
        assert (r["margin"][on_edge] == 0).all() and on_edge.sum() == c.n_edge
        n_edge += c.n_edge; n_events += r["n_events"]; n_one += c.kinds.count("one")
        g64 += int(((lg[:, 1] >> 6) != (lg[:, 2] >> 6)).sum()); g4096 += int(((lg[:, 1] >> 12) != (lg[:, 2] >> 12)).sum())
        chunk += int((lg[:, 0] % nn >= 64).sum()); high += int((lg[:, 1] >= 262144).sum())
        if N == 2:
            assert r["n_events"] == 1 and r["dry"]                      # one event, then error 7 with n_events_out == 1
        d = OnDevice(c)
        rc, n, ex, log, et = aid(hip, d, N, nn, c.draws, 0)
        assert n == len(log)
        check_against_reference(c, rc, log, ex, et, *d.state())
        if not r["dry"] and seed == seeds[0]:
            # the table and tree the call left behind, as far as the next call's picks show them
            more = np.array([0.0, 1.0, 0.37, 1.0, 1.0 - 2.0 ** -53, 1.0, 0.81, 1.0, 1.0, 1e-300])
            want = ref.run(None, None, None, None, None, more, loop=copy.deepcopy(r["loop"]))
            rc, n, ex, log, et = aid(hip, d, N, nn, more, 1)
            assert want["n_events"] == 5 and np.array_equal(log, want["log"]) and (rc, ex) == (0, 0) and abs(et / want["dt"] - 1) <= 1e-12
            assert np.array_equal(d.state()[0], want["element"]) and np.array_equal(d.state()[1], want["charge"])
    print("shape %s: %d events, %d on an edge, %d draws of 1.0, pairs across 64-row groups %d, across 4096-row groups %d, picks in slot chunk >= 1 %d, "
          "in rows >= 262144 %d" % (shape, n_events, n_edge, n_one, g64, g4096, chunk, high))
    assert n_edge >= 20 and n_one >= 1 and n_events >= want_events
    assert g64 >= 1 or N <= 64
    assert g4096 >= 1 or N <= 4096
    assert chunk >= 1 or shape not in ((65, 65), (257, 130))
    assert high >= 1 or N <= 262144


@pytest.mark.parametrize("shape", [(63, 3), (257, 130), (262145, 2)])
def test_resume_in_batches(hip, shape):
    N, nn = shape
    c = case(N, nn, 0)
    d = OnDevice(c)
    for n_uniform in (2, 4, 128, 3):
        d.reset()
        rc, log, ex, et, calls = batched(hip, d, c, n_uniform)
        print("shape %s n_uniform %d: %d calls" % (shape, n_uniform, calls))
        assert calls >= c.ref["n_events"] // (n_uniform // 2)
        check_against_reference(c, rc, log, ex, et, *d.state())


@pytest.mark.parametrize("shape", [(65, 65), (4097, 2)])
def test_same_bytes_twice(hip, shape):
    N, nn = shape
    c = case(N, nn, 0)
    outs = []
    for rep in range(2):
        d = OnDevice(c)
        rc, n, ex, log, et = aid(hip, d, N, nn, c.draws, 0)
        outs.append((rc, n, ex, log.tobytes(), np.float64(et).tobytes(), d.state()[0].tobytes(), d.state()[1].tobytes()))
    assert outs[0] == outs[1]


# ---- 2. production layer ----------------------------------------------------------------------------------------------------------------
def synthetic(N, nn, seed):
    """A random physical state (the recipe of test_gpu_event_temperature._synthetic) on an index the loop may run on: symmetric, padded with -1.
    Sites on a jittered 3 A grid, so that no pair is close enough for its self-interaction term to overflow exp()."""
    rng = np.random.default_rng(seed + 1000 * N + nn)
    m = int(np.ceil(N ** (1 / 3)))
    cell = rng.permutation(m ** 3)[:N]
    xyz = 3.0 * np.stack([cell // (m * m), cell // m % m, cell % m], axis=1) + rng.uniform(-0.5, 0.5, (N, 3))
    neigh = cases.ring_index(N, rng) if nn == 2 else cases.graph_index(N, nn, rng, 0.6)
    cases.check_index(neigh, N, nn)
    h = dict(site_x=xyz[:, 0].copy(), site_y=xyz[:, 1].copy(), site_z=xyz[:, 2].copy(),
             site_potential_boundary=0.5 * rng.standard_normal(N), site_potential_charge=0.2 * rng.standard_normal(N),
             site_element=rng.integers(0, 5, N).astype(np.int32), site_charge=rng.integers(-2, 3, N).astype(np.int32),
             site_layer=rng.integers(0, 5, N).astype(np.int32), neigh_idx=neigh,
             lattice=np.array([3.0 * m] * 3), T_bg=np.array([300.0]), freq=np.array([1e13]), sigma=np.array([3.5e-10]), k=np.array([8.987552e9 / 23.0]))
    E = [rng.uniform(0.0, 3.0, 5) for _ in range(4)]
    T = rng.uniform(250.0, 900.0, N)
    T[rng.random(N) < 0.3] = 300.0
    draws = rng.random(128)
    return h, E, T, draws


# seeds for which the reference shows every margin above 1e-9 Psum (tried beforehand with event_temp_ref.slot_tables in place of the device's table)
PRODUCTION = {(65, 65): 2, (257, 130): 5, (4097, 2): 3}


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("shape", list(PRODUCTION))
def test_production_step_is_the_aid_and_the_reference(hip, shape, mode):
    from devicekmc_amd.host import _ptr
    from test_gpu_event_temperature import _restore, build_T, dev_T
    host, L = hip
    N, nn = shape
    torch = _torch()
    try:
        h, E, T, draws = synthetic(N, nn, PRODUCTION[shape])
        t = {k_: torch.as_tensor(v).to("cuda:0") for k_, v in h.items()}
        assert L.dkmc_copy_to_const_memory(*[e.ctypes.data_as(C.c_void_p) for e in E], 5) == 0
        Td = dev_T(T)
        _, P, P_t = build_T(L, N, nn, t, mode, Td if mode else None)
        assert np.isfinite(P).all() and (P >= 0).all() and (P > 0).sum() > 0
        # the reference on the read-back table: no draw within 1e-9 Psum of an edge, so none is exempt
        r = ref.run(P.astype(np.longdouble), h["neigh_idx"], h["site_element"], h["site_charge"], 1e13, draws)
        rel = r["margin"] / np.array(r["loop"].psums)
        print("shape %s mode %d: %d events, exhausted %s, dry %s, smallest margin %.3g Psum" % (shape, mode, r["n_events"], r["exhausted"], r["dry"], rel.min()))
        assert r["n_events"] >= 3 and (rel > 1e-9).all()
        # the production step
        host._use_stream("cuda:0")
        el, q = t["site_element"].clone(), t["site_charge"].clone()
        n, ex, et = C.c_int(-1), C.c_int(-1), C.c_double(-1.0)
        log = np.full((64, 4), -9, dtype=np.int32)
        L.dkmc_set_event_temperature(mode)
        rc = L.dkmc_execute_kmc_step_gpu(N, nn, _ptr(t["neigh_idx"]), _ptr(t["site_layer"]), _ptr(t["lattice"]), 0, _ptr(t["T_bg"]), _ptr(t["freq"]),
                                         _ptr(t["sigma"]), _ptr(t["k"]), _ptr(t["site_x"]), _ptr(t["site_y"]), _ptr(t["site_z"]),
                                         _ptr(t["site_potential_boundary"]), _ptr(t["site_potential_charge"]), _ptr(Td), _ptr(el), _ptr(q),
                                         draws.ctypes.data_as(C.c_void_p), len(draws), 0, C.byref(n), C.byref(ex), log.ctypes.data_as(C.c_void_p), C.byref(et))
        L.dkmc_set_event_temperature(0)
        if rc:
            assert rc == 7, L.dkmc_last_error()
            L.dkmc_clear_error()
        # the aid on the table the build gives: the same table, the same summation order -- the same bits
        d = OnDevice.__new__(OnDevice)
        d.neigh, d.table, d.freq = t["neigh_idx"], P_t, t["freq"]
        d.element, d.charge = t["site_element"].clone(), t["site_charge"].clone()
        arc, an, aex, alog, aet = aid(hip, d, N, nn, draws, 0)
        assert (rc, n.value, ex.value) == (arc, an, aex) and log[:an].tobytes() == alog.tobytes() and (log[an:] == -9).all()
        assert np.float64(et.value).tobytes() == np.float64(aet).tobytes()
        assert torch.equal(el, d.element) and torch.equal(q, d.charge)
        # ... and the reference's log, every draw
        assert an == r["n_events"] and np.array_equal(alog, r["log"]) and aex == int(r["exhausted"]) and arc == (7 if r["dry"] else 0)
        assert np.array_equal(el.cpu().numpy(), r["element"]) and np.array_equal(q.cpu().numpy(), r["charge"])
    finally:
        _restore(L)


# ---- 3. the aid leaves production alone -------------------------------------------------------------------------------------------------
def test_aid_leaves_the_next_step_alone(cell_2p5, hip):
    """Two supersteps of the 2.5 nm cell give the same event log, dt, elements and charges with and without an aid call in between."""
    from devicekmc_amd import params as pm
    from test_gpu_parity import get, make_pair

    def sequence(with_aid):
        p = pm.KMCParameters()
        dev, sim, gb, o = make_pair(cell_2p5, p, hip)
        out = []
        for k in range(2):
            dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, k)
            _, dt = sim.executeKMCStep(gb, dev, want_log=True)
            dev.updatePower(gb, p, Vd)
            out.append((sim.last_event_log.tobytes(), dt, get(gb, "site_element").tobytes(), get(gb, "site_charge").tobytes()))
            if with_aid and k == 0:
                c = case(65, 65, 0)
                rc, n, ex, log, et = aid(hip, OnDevice(c), 65, 65, c.draws, 0)
                assert n == c.ref["n_events"] > 0
        assert len(sim.last_event_log) > 0
        return out

    assert sequence(True) == sequence(False)
