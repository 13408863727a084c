"""The split polynomial preconditioner in the slab-distributed block-CG (dkmc_set_x_slab_poly; csrc/xtb_slab.inc), run with VIRTUAL ranks.

dkmc_xtb_emulate_slabs runs N virtual ranks inside one process on the X of the 85 071-site device (every virtual rank with its own panels, lists
and exchange buffers, every exchange a device copy) and compares with the one-GPU block-CG -- with the switch on, the one-GPU PRECONDITIONED loop.
The emulation itself fails unless all virtual ranks leave the loop at the same sweep and end with the same bits.
"""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _resident_x():
    """One superstep of the 85 071-site device at cg_tol = 1e-10: leaves its X resident for the emulation."""
    import torch
    from devicekmc_amd import host, lib, params, structure
    lib.load().dkmc_set_x_format(1)
    s = structure.load_structure(os.path.join(GOLDEN, "device_7.5nm.npz"))
    p = params.KMCParameters(rnd_seed=5, lattice=(108.984050, 76.725000, 76.725000), num_atoms_first_layer=1296,
                             num_atoms_contact=12960, A=76.725e-10 * 76.725e-10)
    p.cg_tol = 1e-10
    p.solve_heating_global = True; p.rnd_seed_kmc = 1
    dev = host.Device(s, p)
    sim = host.KMCProcess(dev, p.freq)
    gb = dev.make_gpubuf("cuda:0")
    dev.setLaplacePotential(gb, p, 5.0); gb.sync_HostToGPU(dev)
    dev.updateCharge(gb); dev.updatePotential(gb, p, 5.0, 0)
    _, dt = sim.executeKMCStep(gb, dev)
    dev.updatePower(gb, p, 5.0); dev.updateTemperature(gb, p, dt)
    torch.cuda.synchronize()
    return dict(host.get_stats())


def _emulate(L, nr, time_rank=None, tol=1e-10):
    from devicekmc_amd import lib
    rd, it_s, it_r = C.c_double(-1), C.c_int(0), C.c_int(0)
    us, xd, mm = (C.c_double * 8)(), (C.c_longlong * 3)(), (C.c_int * 2)()
    tr = (nr // 2 if nr > 1 else -1) if time_rank is None else time_rank
    lib.check(L.dkmc_xtb_emulate_slabs(nr, 16, tol, tr, 0, C.byref(rd), C.byref(it_s), C.byref(it_r), us, xd, mm))
    ex, hd, nm = C.c_int(-1), C.c_longlong(-1), C.c_double(-1)
    lib.check(L.dkmc_xtb_slab_last(C.byref(ex), C.byref(hd), C.byref(nm)))
    return dict(rel=rd.value, sweeps=it_s.value, ref=it_r.value, us=list(us), xd=list(xd), ex=ex.value, halo=hd.value, nmul_us=nm.value)


def test_slab_poly_switch_defaults_off():
    """The switch is opt-in: 0 in a fresh process; the setter clamps to 0 / 1 (no GPU needed: the library only loads)."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from devicekmc_amd import lib\n"
            "L = lib.load(); v0 = L.dkmc_get_x_slab_poly(); L.dkmc_set_x_slab_poly(5); v1 = L.dkmc_get_x_slab_poly();"
            " L.dkmc_set_x_slab_poly(0); print(v0, v1, L.dkmc_get_x_slab_poly())\n" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["0", "1", "0"], out.stdout


@pytest.mark.gpu
def test_slab_poly_virtual_ranks_match_one_gpu_preconditioned():
    """Switch on, x_poly = 8: for N = 1, 2, 5, 8 virtual ranks the distributed loop on L A L gives the one-GPU preconditioned solution to 1e-8
    of the largest entry and its sweep count to within max(2, 5 %); it needs less than half the sweeps of the plain slab loop; it runs
    2 d + 3 exchanges per sweep, each halo exchange no larger than exchange 3."""
    import __graft_entry__ as g
    g.build()
    from devicekmc_amd import lib
    L = lib.load()
    _resident_x()
    assert L.dkmc_get_x_poly() == 8
    try:
        for nr in (1, 2, 5, 8):
            L.dkmc_set_x_slab_poly(0)
            plain = _emulate(L, nr)
            L.dkmc_set_x_slab_poly(1)
            pre = _emulate(L, nr)
            print("N=%d: preconditioned %d sweeps (one GPU %d, rel diff %.2e), plain %d; %d exchanges per sweep, %d halo doubles, nmul %.1f us, kernel us %s"
                  % (nr, pre["sweeps"], pre["ref"], pre["rel"], plain["sweeps"], pre["ex"], pre["halo"], pre["nmul_us"], [round(x, 1) for x in pre["us"]]))
            assert 0 <= pre["rel"] <= 1e-8, (nr, pre)
            assert abs(pre["sweeps"] - pre["ref"]) <= max(2, pre["ref"] // 20), (nr, pre)
            assert pre["sweeps"] < 0.5 * plain["sweeps"], (nr, pre["sweeps"], plain["sweeps"])
            if nr > 1:
                assert pre["ex"] == 2 * 8 + 3 and plain["ex"] == 3, (pre["ex"], plain["ex"])
                assert 0 < pre["halo"] <= pre["xd"][2], (pre["halo"], pre["xd"])
                assert pre["nmul_us"] > 0 and pre["us"][3] > 0 and pre["us"][6] > 0
        # other degrees: the same coefficients as the one-GPU loop.  (At d = 4 and 1e-10 the true residual after the first round lies at the
        # rounding floor of A y - b, where the summation order alone decides whether a second round runs -- measured: 41 against 48 sweeps at
        # 4e-13 of each other; the sweep counts are compared at 1e-9.)
        for d in (4, 16):
            L.dkmc_set_x_poly(d)
            pre = _emulate(L, 2, tol=1e-9)
            print("N=2, d=%d: %d sweeps (one GPU %d), rel diff %.2e" % (d, pre["sweeps"], pre["ref"], pre["rel"]))
            assert 0 <= pre["rel"] <= 1e-8, (d, pre)
            assert abs(pre["sweeps"] - pre["ref"]) <= max(2, pre["ref"] // 20), (d, pre)
            assert pre["ex"] == 2 * d + 3
    finally:
        L.dkmc_set_x_slab_poly(0)
        L.dkmc_set_x_poly(8)


@pytest.mark.gpu
def test_slab_poly_csr_form_same_bits():
    """x_nmul_form(0) (N products on the CSR of Xs, row-list variant of k_xtb_nmul) gives the same sweeps and the same bits as the packed form: the
    one-GPU reference is the same in both runs (its two forms agree bit for bit, test_gpu_nmul_form.py), so the deviation of the distributed
    solution from it must be the same double."""
    import __graft_entry__ as g
    g.build()
    from devicekmc_amd import lib
    L = lib.load()
    _resident_x()
    out = {}
    try:
        L.dkmc_set_x_slab_poly(1)
        for form in (1, 0):
            L.dkmc_set_x_nmul_form(form)
            out[form] = _emulate(L, 2, time_rank=-1)
    finally:
        L.dkmc_set_x_nmul_form(1)
        L.dkmc_set_x_slab_poly(0)
    print("nmul form 1 / 0:", out[1], out[0])
    assert out[0]["sweeps"] == out[1]["sweeps"] and out[0]["ref"] == out[1]["ref"]
    assert out[0]["rel"] == out[1]["rel"] and 0 <= out[1]["rel"] <= 1e-8


@pytest.mark.gpu
def test_slab_poly_off_is_unchanged():
    """Switch at 0: an N = 2 emulation runs the plain loop (3 exchanges per sweep) and agrees with the one-GPU plain loop as the existing test
    requires; turning the switch on and back off gives the same sweeps and the same deviation from the (deterministic) one-GPU reference, to the
    bit, as before (no state leaks from the preconditioned run)."""
    import __graft_entry__ as g
    g.build()
    from devicekmc_amd import lib
    L = lib.load()
    _resident_x()
    assert L.dkmc_get_x_slab_poly() == 0
    a = _emulate(L, 2, time_rank=-1)
    assert a["ex"] == 3 and 0 <= a["rel"] <= 1e-8 and abs(a["sweeps"] - a["ref"]) <= max(3, a["ref"] // 20), a
    try:
        L.dkmc_set_x_slab_poly(1)
        on = _emulate(L, 2, time_rank=-1)
        assert on["ex"] == 19 and on["sweeps"] < a["sweeps"]
    finally:
        L.dkmc_set_x_slab_poly(0)
    b = _emulate(L, 2, time_rank=-1)
    assert b["ex"] == 3 and b["sweeps"] == a["sweeps"] and b["ref"] == a["ref"]
    assert b["rel"] == a["rel"]
