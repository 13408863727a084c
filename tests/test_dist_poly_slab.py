"""The split polynomial preconditioner in the slab-distributed block-CG (dkmc_set_x_slab_poly; csrc/xtb_slab.inc) with two REAL ranks.

Two ranks share cuda:0 over the host-callback transport (gloo), as in test_dist_sharded.py.  (File name: sorts before test_dist_sharded.py and
every test_gpu_* so that the ranks are spawned from a parent that has not touched the GPU.)
"""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

Vd = 5.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _big_device(tol):
    from devicekmc_amd import host, params, structure
    s = structure.load_structure(os.path.join(GOLDEN, "device_7.5nm.npz"))
    p = params.KMCParameters(rnd_seed=5, lattice=(108.984050, 76.725000, 76.725000), num_atoms_first_layer=1296,
                             num_atoms_contact=12960, A=76.725e-10 * 76.725e-10)
    if tol is not None:
        p.cg_tol = tol
    p.solve_heating_global = True; p.rnd_seed_kmc = 1
    dev = host.Device(s, p)
    sim = host.KMCProcess(dev, p.freq)
    gb = dev.make_gpubuf("cuda:0")
    dev.setLaplacePotential(gb, p, Vd); gb.sync_HostToGPU(dev)
    return p, dev, sim, gb


def _supersteps(nsteps):
    """nsteps supersteps of the 85 071-site device from a fresh state at cg_tol = 1e-10 (tiled X); everything a caller can observe."""
    import torch
    from devicekmc_amd import host
    p, dev, sim, gb = _big_device(1e-10)
    trace, iters = [], []
    for k in range(nsteps):
        dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, k)
        _, dt = sim.executeKMCStep(gb, dev)
        dev.updatePower(gb, p, Vd); dev.updateTemperature(gb, p, dt)
        torch.cuda.synchronize()
        trace.append((dt, dev.imacro, dev.T_bg)); iters.append(host.get_stats()["cg_iters_X"])
    fields = {n: gb.t[n].cpu().numpy().copy() for n in ("site_power", "site_potential_boundary", "site_potential_charge",
                                                        "site_charge", "site_element", "atom_virtual_potentials")}
    return trace, iters, fields, dict(host.get_stats())


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    from devicekmc_amd import lib, parallel
    parallel.init("gloo")
    torch.cuda.set_device(0)
    L = lib.load()
    ref = _supersteps(2) if rank == 0 else None                # one GPU, default arithmetic (preconditioned, d = 8)
    parallel.barrier()
    assert parallel.attach_solver_comm() == "host"
    got_off = _supersteps(2)                                    # slab-distributed, plain loop (default)
    L.dkmc_set_x_slab_poly(1)
    try:
        got_on = _supersteps(2)                                 # slab-distributed on L A L
    finally:
        L.dkmc_set_x_slab_poly(0)
    parallel.detach_solver_comm()
    parallel.barrier()
    q.put((rank, ref, got_off, got_on))
    parallel.finalize()


def test_two_ranks_preconditioned_slab_loop():
    """Two supersteps of the 85 k-site device at cg_tol = 1e-10 with the switch on: the ranks hold the same bits (trace, sweep counts, every
    field); dt, I_macro and T_bg match the one-GPU default run to 1e-8; the sweeps per step are the one-GPU preconditioned count to within
    max(2, 5 %) and less than half of the plain slab loop's."""
    import __graft_entry__ as g
    g.build()
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs: p.start()
    out = sorted((q.get(timeout=900) for _ in range(world)), key=lambda t: t[0])
    for p in procs: p.join(120); assert p.exitcode == 0
    (_, ref, off0, on0), (_, _, off1, on1) = out
    print("sweeps per step: one GPU", ref[1], "slab plain", off0[1], "slab preconditioned", on0[1])
    assert on0[0] == on1[0] and on0[1] == on1[1]
    for n in on0[2]:
        assert np.array_equal(on0[2][n], on1[2][n]), n
    assert on0[3]["comm_ranks"] == 2 and on0[3]["xb_width"] == 16
    for (dt, im, tb), (dt2, im2, tb2) in zip(on0[0], ref[0]):
        assert abs(dt - dt2) <= 1e-8 * dt and abs(im - im2) <= 1e-8 * abs(im) and abs(tb - tb2) <= 1e-8 * tb
    assert np.array_equal(on0[2]["site_element"], ref[2]["site_element"])
    for k, (a, r, pl) in enumerate(zip(on0[1], ref[1], off0[1])):
        assert abs(a - r) <= max(2, r // 20), (k, on0[1], ref[1])
        assert a < 0.5 * pl, (k, on0[1], off0[1])


def _fault_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    from devicekmc_amd import lib, parallel
    from devicekmc_amd.lib import DeviceKMCError
    parallel.init("gloo")
    torch.cuda.set_device(0)
    assert parallel.attach_solver_comm() == "host"
    L = lib.load()
    p, dev, sim, gb = _big_device(None)
    seen = []
    L.dkmc_set_x_slab_poly(1)
    try:
        # on the host side of block-CG iteration 5 (the preconditioned slab loop); clean step
        for phase, it in ((3, 5), (0, 0)):
            dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, 0)
            sim.executeKMCStep(gb, dev)
            if rank == 1 and phase:
                L.dkmc_debug_inject_fault(phase, it)
            try:
                dev.updatePower(gb, p, Vd)
                seen.append((0, dev.imacro))
            except DeviceKMCError as exc:
                seen.append((1, str(exc)))
                L.dkmc_clear_error()
            parallel.barrier()
    finally:
        L.dkmc_set_x_slab_poly(0)
    parallel.detach_solver_comm()
    q.put((rank, seen))
    parallel.finalize()


def test_preconditioned_slab_error_path_returns_on_every_rank():
    """A rank-local failure on the host side of an iteration of the preconditioned slab loop (dkmc_debug_inject_fault(3, 5) on rank 1, an error
    code raised on the host) must not leave the peer in a collective: the failing rank still joins every halo exchange of the sweep, the abort
    word travels with exchanges 1 and 2; both ranks return an error and the next clean superstep gives the same current on both."""
    import __graft_entry__ as g
    g.build()
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_fault_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs: p.start()
    out = sorted((q.get(timeout=600) for _ in range(world)), key=lambda t: t[0])
    for p in procs: p.join(60); assert p.exitcode == 0
    (_, s0), (_, s1) = out
    assert [k for k, _ in s0] == [1, 0] and [k for k, _ in s1] == [1, 0], (s0, s1)
    assert "peer rank" in s0[0][1] and "injected fault (block-CG iteration" in s1[0][1]
    assert s0[1][1] == s1[1][1] and s0[1][1] != 0.0
