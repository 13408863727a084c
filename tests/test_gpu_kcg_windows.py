"""The windowed blocked form of the CG on K (dkmc_set_k_blocked_large, csrc/kcg.hip + csrc/kbw_plan.h): systems above 262 144 device rows, rows in
an internal spatial order, blocks whose window of the direction vector is a few contiguous segments copied into LDS.  Checked against the CSR
positions of the pattern (the default above that size) and the oracle's K, by the project's rule for CG solutions: converged solves or the TRUE
residual, never iteration counts or bits across forms.  The switch is read when a pattern is built, so every test sets it before building the
device and resets it in a `finally`."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Vd = 5.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__ as g
    g.build()
    from devicekmc_amd import host, lib
    return host, lib.load()


def _fresh(name, solve_current=False, cg_tol=None):
    sys.path.insert(0, ROOT)
    from bench import make_workload
    from devicekmc_amd import host
    s, p = make_workload(name)
    if not solve_current:
        p.solve_current = False; p.solve_heating_global = False
    if cg_tol is not None:
        p.cg_tol = cg_tol
    dev = host.Device(s, p, gpu_neighbors="cuda:0")
    sim = host.KMCProcess(dev, p.freq)
    gb = dev.make_gpubuf("cuda:0")
    dev.setLaplacePotential(gb, p, Vd)
    gb.sync_HostToGPU(dev)
    return s, p, dev, sim, gb


def _form(L, gb):
    info = (C.c_longlong * 9)()
    from devicekmc_amd import lib
    lib.check(L.dkmc_kcg_form_info(C.byref(gb.c), info))
    return list(info)


def _oracle_K(s, p, dev, gb):
    """K and rhs of the buffer's current state, assembled by the oracle on the pattern initialize_sparsity published (okmc_k_assemble)."""
    import scipy.sparse as sp
    from oracle import oracle as oc
    from test_gpu_parity import _d2h_i32
    nl = p.num_atoms_first_layer
    m = s.N - 2 * nl
    c = gb.c
    rp, ci = _d2h_i32(c.Device_row_ptr_d, m + 1), _d2h_i32(c.Device_col_indices_d, int(c.Device_nnz))
    lrp, lci = _d2h_i32(c.contact_left_row_ptr, m + 1), _d2h_i32(c.contact_left_col_indices, max(int(c.contact_left_nnz), 1))[:int(c.contact_left_nnz)]
    rrp, rci = _d2h_i32(c.contact_right_row_ptr, m + 1), _d2h_i32(c.contact_right_col_indices, max(int(c.contact_right_nnz), 1))[:int(c.contact_right_nnz)]
    data, rhs = np.zeros(len(ci)), np.zeros(m)
    _p = oc._p
    metals = np.asarray(list(p.metals), dtype=np.int32)
    el32 = np.ascontiguousarray(gb.site_element.cpu().numpy().astype(np.int32))
    q32 = np.ascontiguousarray(gb.site_charge.cpu().numpy().astype(np.int32))
    oc.lib().okmc_k_assemble(s.N, nl, nl, _p(el32), _p(q32), _p(metals), len(metals), C.c_double(p.high_G), C.c_double(p.low_G), 0,
                             _p(rp), _p(ci), _p(lrp), _p(lci), _p(rrp), _p(rci), C.c_double(-Vd / 2), C.c_double(Vd / 2), _p(data), _p(rhs))
    return sp.csr_matrix((data, ci, rp), shape=(m, m)), rhs, nl, m


def _scaled_res(K, rhs, phi):
    return float(np.linalg.norm((K @ phi - rhs) / np.sqrt(K.diagonal())))


@pytest.fixture(scope="module")
def tile10_converged(hip):
    """The first background-potential solve of tile:10 (911 100 K rows, current off) at cg_tol = 1e-10 in three builds of the pattern: switch off
    (CSR positions), switch on (windowed form; solved twice from the same start), switch on with the segment cap forced to 1 (builder refuses)."""
    import torch
    host, L = hip
    out = {}
    try:
        for mode in ("off", "on", "refused"):
            L.dkmc_set_k_blocked_large(0 if mode == "off" else 1)
            L.dkmc_debug_kbw_segment_cap(1 if mode == "refused" else 0)
            s, p, dev, sim, gb = _fresh("tile:10", cg_tol=1e-10)
            form = _form(L, gb)
            dev.updateCharge(gb)
            start = gb.site_potential_boundary.clone()
            dev.updatePotential(gb, p, Vd, 0)
            torch.cuda.synchronize()
            st = host.get_stats()
            rec = dict(form=form, kcg=st["kcg_blocked"], rr=st["cg_rr_K"], phi=gb.site_potential_boundary.cpu().numpy().copy())
            if mode == "on":
                gb.site_potential_boundary.copy_(start)
                dev.updatePotential(gb, p, Vd, 0)
                torch.cuda.synchronize()
                rec["phi2"] = gb.site_potential_boundary.cpu().numpy().copy()
                rec["kcg2"] = host.get_stats()["kcg_blocked"]
            if mode != "refused":
                K, rhs, nl, m = _oracle_K(s, p, dev, gb)
                rec["sres"] = _scaled_res(K, rhs, rec["phi"][nl:nl + m])
            rec["tol"], rec["nl"] = p.cg_tol, p.num_atoms_first_layer
            out[mode] = rec
            del dev, sim, gb
            torch.cuda.empty_cache()
    finally:
        L.dkmc_set_k_blocked_large(0); L.dkmc_debug_kbw_segment_cap(0); L.dkmc_set_cg_tolerance(1e-6)
    return out


def test_tile10_form_selection(tile10_converged):
    on, off = tile10_converged["on"], tile10_converged["off"]
    assert off["kcg"] == 0 and off["form"][0] == 0
    assert on["kcg"] == 2 and on["kcg2"] == 2
    form, rows, R, nb, maxwin, winsum, maxseg, segsum, ints = on["form"]
    assert form == 2 and rows == 911100 and nb * R >= rows > (nb - 1) * R
    assert nb >= 256 and 0 < maxwin <= 14336 and 1 <= maxseg <= 16 and winsum >= rows


def test_tile10_converged_agreement(tile10_converged):
    """cg_tol = 1e-10: the two forms agree to 1e-8 V, and each meets the stop test in the true scaled residual of the oracle's K on the CSR pattern."""
    on, off = tile10_converged["on"], tile10_converged["off"]
    assert np.abs(on["phi"] - off["phi"]).max() <= 1e-8, np.abs(on["phi"] - off["phi"]).max()
    nl = on["nl"]
    assert (on["phi"][:nl] == -Vd / 2).all() and (on["phi"][-nl:] == Vd / 2).all()
    for rec in (on, off):
        assert rec["rr"] <= rec["tol"] ** 2
        assert rec["sres"] <= 10 * rec["tol"], rec["sres"]


def test_tile10_windowed_solve_is_deterministic(tile10_converged):
    on = tile10_converged["on"]
    assert np.array_equal(on["phi"], on["phi2"])


def test_tile10_refused_build_falls_back_to_csr_positions(tile10_converged):
    """With the segment cap forced below what any window needs the builder refuses: the solve runs on the CSR positions, bit for bit as with the switch off."""
    ref, off = tile10_converged["refused"], tile10_converged["off"]
    assert ref["kcg"] == 0 and ref["form"][0] == 0
    assert np.array_equal(ref["phi"], off["phi"])


def test_small_system_keeps_the_blocked_form(hip):
    """At or below 262 144 rows (7.5 nm: 85 071 sites) the pattern keeps today's blocked form whatever the switch says."""
    host, L = hip
    try:
        for on in (0, 1):
            L.dkmc_set_k_blocked_large(on)
            s, p, dev, sim, gb = _fresh("7.5nm")
            assert _form(L, gb)[0] == 1
            dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, 0)
            assert host.get_stats()["kcg_blocked"] == 1, on
    finally:
        L.dkmc_set_k_blocked_large(0)


def test_tile10_default_tolerance_supersteps(hip):
    """Three coupled supersteps of tile:10 (current off) at the library's default tolerance on the windowed form: every K solution meets the stop test in
    the TRUE residual of the oracle's K of that state, and the oracle, fed the GPU's two potentials, builds the same event table and executes the same
    (slot, i, j, type) sequence with the same dt, elements and charges (test_default_tolerance_superstep_7p5's pattern)."""
    import torch
    from oracle import oracle as oc
    host, L = hip
    try:
        L.dkmc_set_k_blocked_large(1)
        s, p, dev, sim, gb = _fresh("tile:10")
        assert p.cg_tol == 1e-6
        o = oc.OracleKMC(s.element, s.x, s.y, s.z, p, neigh=dev.neigh_idx)
        assert np.array_equal(o.element, dev.site_element)
        o.CB_edge[:] = gb.site_CB_edge.cpu().numpy()
        for k in range(3):
            dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, k)
            torch.cuda.synchronize()
            st = host.get_stats()
            assert st["kcg_blocked"] == 2 and st["cg_rr_K"] <= p.cg_tol ** 2, k
            o.update_charge()
            assert np.array_equal(gb.site_charge.cpu().numpy(), o.charge), k
            pb, pc = gb.site_potential_boundary.cpu().numpy().copy(), gb.site_potential_charge.cpu().numpy().copy()
            K, rhs, nl, m = _oracle_K(s, p, dev, gb)
            sres = _scaled_res(K, rhs, pb[nl:nl + m])
            assert sres <= 10 * p.cg_tol, (k, sres)
            o.pot_boundary[:] = pb; o.pot_charge[:] = pc
            _, dt = sim.executeKMCStep(gb, dev, want_log=True)
            odt = o.execute_kmc_step()
            assert np.array_equal(sim.last_event_log, o.last_events["log"]), k
            assert o.last_events["margin"].min() > 1e-9
            assert abs(dt / odt - 1) <= 1e-5, k
            assert np.array_equal(gb.site_element.cpu().numpy(), o.element) and np.array_equal(gb.site_charge.cpu().numpy(), o.charge), k
    finally:
        L.dkmc_set_k_blocked_large(0)


def test_tile20_current_off_first_superstep_windowed(hip):
    """test_tile20_current_off_first_superstep (tests/test_gpu_scale.py) with the K solve on the windowed form: 3 644 400 K rows, the same fixture
    (tests/golden/tile20_current_off.npz) and the same checks and tolerances -- default-tolerance solution within the stop test in the true residual of
    the oracle's K, the converged (1e-12) solution within 1e-6 V of the oracle's own on the sampled sites, and the event sequence, KMC time, elements
    and charges of the first superstep from the GPU's converged potentials."""
    import hashlib
    import torch
    host, L = hip
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    fx = np.load(os.path.join(ROOT, "tests", "golden", "tile20_current_off.npz"))
    try:
        L.dkmc_set_k_blocked_large(1)
        s, p, dev, sim, gb = _fresh("tile:20")
        assert s.N == int(fx["N"]) and p.cg_tol == 1e-6
        assert sha(dev.site_element.astype(np.int32)) == str(fx["element0_sha"])
        form = _form(L, gb)
        assert form[0] == 2 and form[1] == int(fx["K_rows"]), form
        dev.updateCharge(gb)
        charge = gb.site_charge.cpu().numpy()
        assert sha(charge.astype(np.int32)) == str(fx["charge_sha"])
        dev.updatePotential(gb, p, Vd, 0)
        torch.cuda.synchronize()
        st = host.get_stats()
        assert st["kcg_blocked"] == 2 and st["cg_rr_K"] <= p.cg_tol ** 2
        pb, pc = gb.site_potential_boundary.cpu().numpy().copy(), gb.site_potential_charge.cpu().numpy().copy()
        K, rhs, nl, m = _oracle_K(s, p, dev, gb)
        assert _scaled_res(K, rhs, pb[nl:nl + m]) <= 10 * p.cg_tol
        assert (pb[:nl] == -Vd / 2).all() and (pb[-nl:] == Vd / 2).all()
        p.cg_tol = 1e-12
        dev.updatePotential(gb, p, Vd, 1)
        torch.cuda.synchronize()
        st = host.get_stats()
        assert st["kcg_blocked"] == 2 and st["cg_rr_K"] <= 1e-24
        pb2, pc2 = gb.site_potential_boundary.cpu().numpy(), gb.site_potential_charge.cpu().numpy()
        assert np.array_equal(pc2, pc)
        assert np.abs(pb2 - pb).max() <= 0.5
        assert _scaled_res(K, rhs, pb2[nl:nl + m]) <= 1e-9
        ps = fx["pb_sites"]
        dpb = np.abs(pb2[ps] - fx["pb_values"]).max()
        print("tile:20 windowed form: max |phi_gpu - phi_oracle| on the sampled sites (both at 1e-12): %.2e V" % dpb)
        assert dpb <= 1e-6, dpb
        assert np.abs(pc2[ps] - fx["pc_values"]).max() <= 1e-12 * float(fx["pc_absmax"])
        _, dt = sim.executeKMCStep(gb, dev, want_log=True)
        assert np.array_equal(sim.last_event_log, fx["event_log"])
        assert abs(dt / float(fx["event_time"]) - 1) <= 1e-5
        gb.sync_GPUToHost(dev)
        assert sha(dev.site_element.astype(np.int32)) == str(fx["element1_sha"]) and sha(dev.site_charge.astype(np.int32)) == str(fx["charge1_sha"])
    finally:
        L.dkmc_set_k_blocked_large(0); L.dkmc_set_cg_tolerance(1e-6)
