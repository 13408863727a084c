"""Event rates on the local site temperature (dkmc_set_event_temperature) and the rate census (dkmc_event_rate_census) on the GPU, against
the numpy restatement tests/event_temp_ref.py (pinned to the CPU oracle in mode 0 by tests/test_event_temp_ref.py) and the oracle's event loop.
Integer work (types, zero pattern, event logs, counts, argmax) exact; rates within 1e-10 relative, the bound of
test_gpu_parity.test_randomised_event_engine: ln(P / freq) spans -315 ... +450 in mode 0, mode 1 shifts it by at most dT / T_bg, mode 2
shrinks it.  Every test restores mode 0, census off and the layer energies."""
import ctypes as C

import numpy as np
import pytest

import event_temp_ref as er

pytestmark = pytest.mark.gpu

Vd = 5.0
SEEDS = (11, 12, 13)


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


def put(gb, name, arr):
    t = gb.t[name]
    t.copy_(_torch().as_tensor(np.ascontiguousarray(arr)).to(t.dtype))


def get(gb, name):
    return gb.t[name].cpu().numpy()


def _restore(L, p=None):
    from devicekmc_amd import params as pm
    L.dkmc_set_event_temperature(0); L.dkmc_set_event_census(0); L.dkmc_clear_error()
    layers = (p or pm.KMCParameters()).layers
    E = [np.array([getattr(l, f) for l in layers], dtype=np.float64) for f in ("E_gen_0", "E_rec_1", "E_diff_2", "E_diff_3")]
    assert L.dkmc_copy_to_const_memory(*[e.ctypes.data_as(C.c_void_p) for e in E], len(layers)) == 0


class State:
    """One randomised state of the 2.5 nm cell (test_randomised_event_engine's, by seed) on the device and in the oracle, with the ball field."""

    def __init__(self, cell, hip, seed):
        from devicekmc_amd import params as pm
        from oracle import oracle as oc
        host, L = hip
        self.p = p = pm.KMCParameters(); p.rnd_seed_kmc = seed
        self.seed = seed
        self.dev = host.Device(cell, p)
        self.gb = self.dev.make_gpubuf("cuda:0")
        self.dev.setLaplacePotential(self.gb, p, Vd)
        self.gb.sync_HostToGPU(self.dev)
        o = oc.OracleKMC(cell.element, cell.x, cell.y, cell.z, p)
        self.el, self.pb, self.pc = er.randomised_state(seed, o.element, o.x)
        o.element[:] = self.el; o.update_charge()
        self.q = o.charge.copy()
        o.pot_boundary[:] = self.pb; o.pot_charge[:] = self.pc
        self.o = o
        self.T_bg = float(p.background_temp)
        self.ball = er.ball_field(o.x, o.y, o.z, self.T_bg)
        self.uniform = np.full(o.N, self.T_bg)
        put(self.gb, "site_element", self.el); self.dev.updateCharge(self.gb)      # from the fresh buffers, as the oracle's: exact
        assert np.array_equal(get(self.gb, "site_charge"), self.q)
        self.ref = {0: er.oracle_tables(o, 0)}
        for mode in (1, 2):
            self.ref[mode] = er.oracle_tables(o, mode, self.ball)
        self.reset(hip)

    def reset(self, hip, T=None):
        """The state before any event, on the device and in the oracle; a fresh KMC stream on both."""
        from oracle import oracle as oc
        host, L = hip
        gb, o = self.gb, self.o
        put(gb, "site_element", self.el); put(gb, "site_charge", self.q)
        put(gb, "site_potential_boundary", self.pb); put(gb, "site_potential_charge", self.pc)
        put(gb, "site_temperature", self.ball if T is None else T)
        gb.t["T_bg"].fill_(self.T_bg)
        o.element[:] = self.el; o.charge[:] = self.q
        o.rng_kmc = oc.OracleRNG(self.seed)
        self.sim = host.KMCProcess(self.dev, self.p.freq)
        self.sim.batch = 64
        return self.sim


_states = {}


@pytest.fixture
def state(request, cell_2p5, hip):
    seed = request.param
    if seed not in _states:
        _states[seed] = State(cell_2p5, hip, seed)
    _restore(hip[1])                                  # the layer energies of the default parameters, whatever ran before
    st = _states[seed]
    st.reset(hip)
    return st


def build_T(L, N, nn, t, mode, T=None, count_bad=False):
    """dkmc_build_event_list_T in `mode` on a dict of device tensors; T: device tensor or None.  Returns (types, P[, n_bad]) on the host."""
    from devicekmc_amd.host import _ptr
    from devicekmc_amd.lib import check
    torch = _torch()
    ev_type = torch.full((N * nn,), -7, dtype=torch.int32, device="cuda:0"); ev_prob = torch.full((N * nn,), -1.0, dtype=torch.float64, device="cuda:0")
    n_bad = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    L.dkmc_set_event_temperature(mode)
    try:
        check(L.dkmc_build_event_list_T(N, nn, _ptr(t["neigh_idx"]), _ptr(t["site_layer"]), _ptr(t["lattice"]), int(t.get("pbc", 0)), _ptr(t["T_bg"]),
                                        _ptr(t["freq"]), _ptr(t["sigma"]), _ptr(t["k"]), _ptr(t["site_x"]), _ptr(t["site_y"]), _ptr(t["site_z"]),
                                        _ptr(t["site_potential_boundary"]), _ptr(t["site_potential_charge"]), _ptr(t["site_element"]),
                                        _ptr(t["site_charge"]), _ptr(ev_type), _ptr(ev_prob), _ptr(T) if T is not None else None,
                                        _ptr(n_bad) if count_bad else None))
        torch.cuda.synchronize()
    finally:
        L.dkmc_set_event_temperature(0)
    out = (ev_type.cpu().numpy(), ev_prob.cpu().numpy())
    return out + (int(n_bad.item()),) if count_bad else out + (ev_prob,)


def dev_T(arr):
    return _torch().as_tensor(np.ascontiguousarray(arr, dtype=np.float64)).to("cuda:0")


def compare_tables(gt, gp, rt, rp):
    """types exact, same zero pattern, same finite pattern, rates within 1e-10 relative."""
    assert np.array_equal(gt, rt)
    assert np.array_equal(gp > 0, rp > 0) and np.array_equal(np.isfinite(gp), np.isfinite(rp))
    m = (rp > 0) & np.isfinite(rp)
    err = np.abs(gp[m] / rp[m] - 1).max() if m.any() else 0.0
    print("slots %d live %d max relative error %.3g" % (len(rp), m.sum(), err))
    assert err <= 1e-10
    assert (gp[~m & np.isfinite(rp)] == 0).all()


# ---- 1. the table on physical states ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", SEEDS, indirect=True)
def test_table_physical_states(state, hip):
    host, L = hip
    st = state
    try:
        N, nn = st.dev.N, st.dev.max_num_neighbors
        Tb = dev_T(st.ball)
        for cls in range(4):
            assert (st.ref[0][0] == cls).sum() > 0, cls
        gt0, gp0, _ = build_T(L, N, nn, st.gb.t, 0, None)
        compare_tables(gt0, gp0, *st.ref[0][:2])
        for mode in (1, 2):
            gt, gp, _ = build_T(L, N, nn, st.gb.t, mode, Tb)
            rt, rp, n_bad = st.ref[mode]
            assert n_bad == 0
            compare_tables(gt, gp, rt, rp)
            moved = (gp != gp0).sum()
            print("seed %d mode %d: %d slots differ from mode 0" % (st.seed, mode, moved))
            assert moved >= 900 and (rp != st.ref[0][1]).sum() >= 900
    finally:
        _restore(L)


# ---- 2. bitwise identities on the device --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", SEEDS, indirect=True)
def test_bitwise_identities(state, hip):
    host, L = hip
    st = state
    try:
        N, nn = st.dev.N, st.dev.max_num_neighbors
        Tu, Tb = dev_T(st.uniform), dev_T(st.ball)
        t0, p0, _ = build_T(L, N, nn, st.gb.t, 0, Tu)
        t0b, p0b, _ = build_T(L, N, nn, st.gb.t, 0, Tb)
        t0n, p0n, _ = build_T(L, N, nn, st.gb.t, 0, None)                       # mode 0 never dereferences the pointer
        assert np.array_equal(p0, p0b) and np.array_equal(t0, t0b) and np.array_equal(p0, p0n) and np.array_equal(t0, t0n)
        T_s, cls = er.deciding_temperature(st.o.neigh, st.o.element, st.ball)
        cold = ~(T_s != st.T_bg)                                               # T_s == T_bg, and the slots without a class
        assert ((cls != er.EV_NULL) & cold).sum() > 1000 and ((cls != er.EV_NULL) & ~cold).sum() >= 900
        for mode in (1, 2):
            t, p, _ = build_T(L, N, nn, st.gb.t, mode, Tu)
            assert np.array_equal(t, t0) and np.array_equal(p, p0)              # (a)
            t, p, _ = build_T(L, N, nn, st.gb.t, mode, Tb)
            assert np.array_equal(t, t0) and np.array_equal(p[cold], p0[cold])  # (b)
            assert (p[~cold] != p0[~cold]).sum() >= 900
    finally:
        _restore(L)


# ---- 3. analytic cross-check, independent of the restatement -----------------------------------------------------------------------
@pytest.mark.parametrize("state", SEEDS, indirect=True)
def test_analytic_cross_check(state, hip):
    host, L = hip
    st = state
    try:
        N, nn = st.dev.N, st.dev.max_num_neighbors
        Tb = dev_T(st.ball)
        _, p0, _ = build_T(L, N, nn, st.gb.t, 0, None)
        _, p1, _ = build_T(L, N, nn, st.gb.t, 1, Tb)
        _, p2, _ = build_T(L, N, nn, st.gb.t, 2, Tb)
        T_s, cls = er.deciding_temperature(st.o.neigh, st.o.element, st.ball)
        m = (p0 > 0) & np.isfinite(p0)
        assert m.sum() > 3000 and (T_s[m] > st.T_bg).sum() >= 900
        freq = st.p.freq
        e1 = np.abs(p1[m] / p0[m] / np.exp((T_s[m] - st.T_bg) / st.T_bg) - 1).max()
        a, b = T_s[m] * np.log(p2[m] / freq), st.T_bg * np.log(p0[m] / freq)
        z = b == 0                                                               # EA is exactly 0 (recombination: E0 = 0, equal charges): both sides 0
        assert (a[z] == 0).all()
        e2 = np.abs(a[~z] / b[~z] - 1).max()
        print("mode 1 ratio error %.3g, mode 2 exponent error %.3g" % (e1, e2))
        assert e1 <= 1e-10 and e2 <= 1e-10
    finally:
        _restore(L)


# ---- 4. event sequences ---------------------------------------------------------------------------------------------------------------
def _compare_step(sim, o, dt, odt, gb, max_exempt=None):
    n = o.last_events["n"]
    safe = o.last_events["margin"] > 1e-9                                       # draws within rounding distance of a bucket edge are exempt
    k = n if safe.all() else int(np.argmin(safe))
    if max_exempt is not None:
        assert k >= n - max_exempt
    assert np.array_equal(sim.last_event_log[:k], o.last_events["log"][:k])
    if safe.all():
        assert len(sim.last_event_log) == n and abs(dt / odt - 1) <= 1e-9
        assert np.array_equal(get(gb, "site_element"), o.element) and np.array_equal(get(gb, "site_charge"), o.charge)
    return bool(safe.all())


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("state", SEEDS, indirect=True)
def test_event_sequences(state, hip, mode):
    host, L = hip
    st = state
    try:
        o = st.o
        # the mode-0 log of the same seed, by the oracle alone
        o.execute_kmc_step(ev=(st.ref[0][0].copy(), st.ref[0][1].copy()))
        log0 = o.last_events["log"].copy()
        sim = st.reset(hip)
        st.p.event_temperature = mode
        _, dt = sim.executeKMCStep(st.gb, st.dev, want_log=True)
        odt = o.execute_kmc_step(ev=(st.ref[mode][0].copy(), st.ref[mode][1].copy()))
        n = o.last_events["n"]
        print("seed %d mode %d: %d events, smallest margin %.3g" % (st.seed, mode, n, o.last_events["margin"].min()))
        # the conditions the inputs were chosen for (checked with the oracle alone beforehand): every draw safe, a long sequence, not mode 0's
        assert (o.last_events["margin"] > 1e-9).all() and n >= 100
        assert n != len(log0) or not np.array_equal(o.last_events["log"], log0)
        assert _compare_step(sim, o, dt, odt, st.gb)
        assert sim.last_n_events == n and L.dkmc_get_event_temperature() == mode
    finally:
        st.p.event_temperature = 0
        _restore(L)


# ---- 5. coupled loop -------------------------------------------------------------------------------------------------------------------
def test_coupled_loop(cell_2p5, hip):
    from devicekmc_amd import params as pm
    from oracle import oracle as oc
    host, L = hip
    p = pm.KMCParameters(); p.solve_heating_local = True; p.cg_tol = 1e-10; p.event_temperature = 2
    try:
        dev = host.Device(cell_2p5, p); sim = host.KMCProcess(dev, p.freq)
        gb = dev.make_gpubuf("cuda:0")
        dev.setLaplacePotential(gb, p, Vd)
        gb.sync_HostToGPU(dev)
        o = oc.OracleKMC(cell_2p5.element, cell_2p5.x, cell_2p5.y, cell_2p5.z, p)
        assert np.array_equal(get(gb, "site_element"), o.element)
        dev.constructLaplacian(gb, p)
        start = er.ball_field(o.x, o.y, o.z, p.background_temp)
        put(gb, "site_temperature", start)
        for step in range(3):
            dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, step)
            # the reference table from the fields as they are on the device at this moment
            o.element[:] = get(gb, "site_element"); o.charge[:] = get(gb, "site_charge")
            o.pot_boundary[:] = get(gb, "site_potential_boundary"); o.pot_charge[:] = get(gb, "site_potential_charge")
            T = get(gb, "site_temperature"); T_bg = float(gb.T_bg.item())
            rt, rp, n_bad = er.oracle_tables(o, 2, T, T_bg=T_bg)
            assert n_bad == 0 and np.isfinite(rp).all()
            _, dt = sim.executeKMCStep(gb, dev, want_log=True)
            odt = o.execute_kmc_step(ev=(rt.copy(), rp.copy()))
            print("step %d: %d events, T_bg %.6f, hottest site %.3f K" % (step, o.last_events["n"], T_bg, T.max()))
            assert o.last_events["n"] >= 1
            _compare_step(sim, o, dt, odt, gb, max_exempt=1)
            dev.updatePower(gb, p, Vd)
            dev.site_element = get(gb, "site_element")
            dev.updateTemperature(gb, p, dt)
            T_after = get(gb, "site_temperature")
            assert np.isfinite(T_after).all() and not np.array_equal(T_after, start)      # the heat model ran in between
            assert not np.array_equal(T_after, T)
    finally:
        _restore(L)


# ---- 6. synthetic shapes --------------------------------------------------------------------------------------------------------------
SHAPES = [(5, 1), (257, 64), (257, 65), (1000, 130)]


def _synthetic(N, nn, seed=3):
    """Random sites, elements, charges, potentials, layers and layer energies; a random padded index with entries < 0 and >= N."""
    torch = _torch()
    rng = np.random.default_rng(seed + 1000 * N + nn)
    h = dict(site_x=rng.uniform(0, 14, N), site_y=rng.uniform(0, 14, N), site_z=rng.uniform(0, 14, N),
             site_potential_boundary=0.5 * rng.standard_normal(N), site_potential_charge=0.2 * rng.standard_normal(N),
             site_element=rng.integers(0, 5, N).astype(np.int32), site_charge=rng.integers(-2, 3, N).astype(np.int32),
             site_layer=rng.integers(0, 5, N).astype(np.int32), neigh_idx=rng.integers(-3, N + 3, N * nn).astype(np.int32),
             lattice=np.array([14.0, 14.0, 14.0]), T_bg=np.array([300.0]), freq=np.array([1e13]), sigma=np.array([3.5e-10]), k=np.array([8.987552e9 / 23.0]))
    if N == 5:      # five sites must still meet every class: (DEFECT, O), (Od, V), (V, O), (Od, DEFECT)
        h["site_element"] = np.array([0, 3, 1, 2, 0], dtype=np.int32); h["neigh_idx"] = np.array([1, 3, 4, 1, -1], dtype=np.int32)
        h["neigh_idx"][2] = 3
    E = [rng.uniform(0.0, 3.0, 5) for _ in range(4)]
    T = rng.uniform(250.0, 900.0, N)
    T[rng.random(N) < 0.3] = 300.0                                              # some deciding sites exactly at T_bg
    t = {k_: torch.as_tensor(v).to("cuda:0") for k_, v in h.items()}
    return h, t, E, T


def _synthetic_ref(h, E, mode, T):
    return er.slot_tables(mode, h["neigh_idx"], h["site_layer"], h["lattice"], 0, 300.0, 1e13, 3.5e-10, 8.987552e9 / 23.0, h["site_x"], h["site_y"],
                          h["site_z"], h["site_potential_boundary"], h["site_potential_charge"], h["site_element"], h["site_charge"], *E, temperature=T)


@pytest.mark.parametrize("shape", SHAPES)
def test_synthetic_shapes(hip, shape):
    host, L = hip
    N, nn = shape
    try:
        h, t, E, T = _synthetic(N, nn)
        assert (h["neigh_idx"] < 0).any() and (N == 5 or (h["neigh_idx"] >= N).any())
        assert L.dkmc_copy_to_const_memory(*[e.ctypes.data_as(C.c_void_p) for e in E], 5) == 0
        Td = dev_T(T)
        for mode in (0, 1, 2):
            gt, gp, _ = build_T(L, N, nn, t, mode, Td if mode else None)
            rt, rp, n_bad = _synthetic_ref(h, E, mode, T)
            assert n_bad == 0 and (rt != er.EV_NULL).sum() > 0
            if N > 5:
                assert all((rt == c).sum() > 0 for c in range(4))
            compare_tables(gt, gp, rt, rp)
    finally:
        _restore(L)


# ---- 7. census ------------------------------------------------------------------------------------------------------------------------
def check_census(host, neigh_t, nn, el_t, P_t, T_t, neigh, el, P, T):
    """Counts, argmax, max and non-finite count exact; each sum within n_c 2^-52 fsum (all terms >= 0: bounds any order); same bits twice;
    with a null temperature info[8..11] are zero and everything else is unchanged."""
    ref = er.census(neigh, el, P, T)
    got = host.event_rate_census(neigh_t, nn, el_t, P_t, T_t)["info16"]
    again = host.event_rate_census(neigh_t, nn, el_t, P_t, T_t)["info16"]
    assert np.array_equal(np.array(got), np.array(again), equal_nan=True)
    for q in (0, 1, 2, 3, 12, 13, 14, 15):
        assert got[q] == ref[q], (q, got[q], ref[q])
    for c in range(4):
        for q in (4 + c, 8 + c):
            print("census entry %d: got %.17g ref %.17g n %d" % (q, got[q], ref[q], ref[c]))
            assert abs(got[q] - ref[q]) <= ref[c] * 2.0 ** -52 * ref[q]
    bare = host.event_rate_census(neigh_t, nn, el_t, P_t, None)["info16"]
    assert bare[8:12] == [0.0] * 4 and bare[:8] == got[:8] and bare[12:] == got[12:]
    return got


@pytest.mark.parametrize("state", SEEDS, indirect=True)
def test_census_physical(state, hip):
    host, L = hip
    st = state
    try:
        N, nn = st.dev.N, st.dev.max_num_neighbors
        Tb = dev_T(st.ball)
        _, gp, P_t = build_T(L, N, nn, st.gb.t, 2, Tb)
        info = check_census(host, st.gb.t["neigh_idx"], nn, st.gb.t["site_element"], P_t, Tb, st.o.neigh, st.el, gp, st.ball)
        assert info[15] > 3000 and all(info[c] > 0 for c in range(4))
        d = host._census_dict(info)
        assert all(st.T_bg * (1 - 1e-12) <= d["mean_temperature"][c] <= (st.T_bg + 300.0) * (1 + 1e-12) for c in host.EVENT_CLASSES)
        if st.seed == 11:
            # two inf entries planted (and a NaN): counted, excluded from everything else
            bad = gp.copy(); live = np.flatnonzero(gp > 0)
            bad[live[3]] = np.inf; bad[live[-2]] = np.inf; bad[7] = np.nan
            got = check_census(host, st.gb.t["neigh_idx"], nn, st.gb.t["site_element"], dev_T(bad), Tb, st.o.neigh, st.el, bad, st.ball)
            assert got[14] == 3 and got[15] == info[15] - 2
            # an all-zero table
            zero = check_census(host, st.gb.t["neigh_idx"], nn, st.gb.t["site_element"], dev_T(np.zeros(N * nn)), Tb, st.o.neigh, st.el, np.zeros(N * nn), st.ball)
            assert zero[:13] == [0.0] * 13 and zero[13] == -1 and zero[14] == 0 and zero[15] == 0
            # the switch: the step's own census is the standalone census of the table of dkmc_build_event_list_T
            st.p.event_temperature, st.p.event_census = 2, True
            sim = st.reset(hip)
            sim.executeKMCStep(st.gb, st.dev)
            assert sim.last_event_census["info16"] == info and sim.last_event_census["n_live"] == int(info[15])
            assert sim.last_event_census["rate_total"] == info[4] + info[5] + info[6] + info[7]
            st.p.event_census = False
            sim = st.reset(hip)
            sim.executeKMCStep(st.gb, st.dev)
            assert sim.last_event_census is None and L.dkmc_get_event_census_on() == 0
    finally:
        st.p.event_temperature, st.p.event_census = 0, False
        _restore(L)


@pytest.mark.parametrize("shape", SHAPES)
def test_census_synthetic(hip, shape):
    host, L = hip
    N, nn = shape
    try:
        h, t, E, T = _synthetic(N, nn)
        assert L.dkmc_copy_to_const_memory(*[e.ctypes.data_as(C.c_void_p) for e in E], 5) == 0
        Td = dev_T(T)
        for mode in (0, 2):
            _, gp, P_t = build_T(L, N, nn, t, mode, Td)
            got = check_census(host, t["neigh_idx"], nn, t["site_element"], P_t, Td, h["neigh_idx"], h["site_element"], gp, T)
            assert got[15] > 0
    finally:
        _restore(L)


# ---- 8. errors --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", [11], indirect=True)
def test_bad_temperatures(state, hip):
    from devicekmc_amd.host import _ptr
    from devicekmc_amd.lib import DeviceKMCError
    host, L = hip
    st = state
    try:
        N, nn = st.dev.N, st.dev.max_num_neighbors
        rt, rp, _ = st.ref[2]
        _, cls = er.deciding_temperature(st.o.neigh, st.o.element, st.ball)
        live = np.flatnonzero((rp > 0) & (cls != er.EV_NULL))
        gen = live[cls[live] == er.EV_GEN]; other = live[cls[live] != er.EV_GEN]
        sites = [int(st.o.neigh.reshape(-1)[gen[0]]), int(other[0] // nn), int(other[-1] // nn)]   # the deciding sites of three live slots
        assert len(set(sites)) == 3
        T = st.ball.copy()
        T[sites[0]], T[sites[1]], T[sites[2]] = np.nan, 0.0, -5.0
        want_t, want_p, want_bad = er.oracle_tables(st.o, 2, T)
        assert want_bad >= 3
        gt, gp, n_bad = build_T(L, N, nn, st.gb.t, 2, dev_T(T), count_bad=True)
        assert n_bad == want_bad
        compare_tables(gt, gp, want_t, want_p)                                   # the type is still written, P = 0
        for mode in (1, 2):
            sim = st.reset(hip, T)
            st.p.event_temperature = mode
            pos = sim.random_generator.n_raw
            with pytest.raises(DeviceKMCError) as ei:
                sim.executeKMCStep(st.gb, st.dev, want_log=True)
            assert "error 16" in str(ei.value) and (" %d event slots" % want_bad) in str(ei.value)
            assert np.array_equal(get(st.gb, "site_element"), st.el) and np.array_equal(get(st.gb, "site_charge"), st.q)
            assert sim.last_n_events == 0 and sim.random_generator.n_raw == pos
        # mode 0 with the same field: the step runs as ever
        sim = st.reset(hip, T)
        st.p.event_temperature = 0
        _, dt = sim.executeKMCStep(st.gb, st.dev, want_log=True)
        odt = st.o.execute_kmc_step(ev=(st.ref[0][0].copy(), st.ref[0][1].copy()))
        assert st.o.last_events["n"] >= 100
        _compare_step(sim, st.o, dt, odt, st.gb)
        # modes 1, 2 without a temperature: bad argument, before any launch
        sim = st.reset(hip)
        g = st.gb
        u = np.ascontiguousarray(sim.random_generator.copy().uniform_batch(128))
        n_ev, exhausted, et = C.c_int(-1), C.c_int(0), C.c_double(0.0)
        L.dkmc_set_event_temperature(2)
        rc = L.dkmc_execute_kmc_step_gpu(N, nn, _ptr(g.neigh_idx), _ptr(g.site_layer), _ptr(g.lattice), 0, _ptr(g.T_bg), _ptr(g.freq), _ptr(g.sigma),
                                         _ptr(g.k), _ptr(g.site_x), _ptr(g.site_y), _ptr(g.site_z), _ptr(g.site_potential_boundary),
                                         _ptr(g.site_potential_charge), None, _ptr(g.site_element), _ptr(g.site_charge),
                                         u.ctypes.data_as(C.c_void_p), len(u), 0, C.byref(n_ev), C.byref(exhausted), None, C.byref(et))
        assert rc == 13 and b"site_temperature" in L.dkmc_last_error()
        L.dkmc_clear_error()
        assert np.array_equal(get(g, "site_element"), st.el)
        torch = _torch()
        P_t = torch.zeros(N * nn, dtype=torch.float64, device="cuda:0")
        args = [N, nn, _ptr(g.neigh_idx), _ptr(g.site_layer), _ptr(g.lattice), 0, _ptr(g.T_bg), _ptr(g.freq), _ptr(g.sigma), _ptr(g.k), _ptr(g.site_x),
                _ptr(g.site_y), _ptr(g.site_z), _ptr(g.site_potential_boundary), _ptr(g.site_potential_charge), _ptr(g.site_element), _ptr(g.site_charge),
                None, _ptr(P_t)]
        assert L.dkmc_build_event_list(*args) == 13                              # it has no temperature
        L.dkmc_clear_error()
        assert L.dkmc_build_event_list_T(*args, None, None) == 13
        L.dkmc_clear_error()
        L.dkmc_set_event_temperature(0)
        assert L.dkmc_build_event_list(*args) == 0 and L.dkmc_build_event_list_T(*args, None, None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(P_t.cpu().numpy(), build_T(L, N, nn, g.t, 0)[1])
    finally:
        st.p.event_temperature = 0
        _restore(L)
