"""The current map (dkmc_set_current_map) in a sharded current solve: two ranks sharing cuda:0 over the host transport, tiled X.  The tile sums of
the two passes are completed by the all-reduce and every rank takes rank 0's bits, as the dissipated power does: the ranks end with the same
arrays, within the derived bounds of the host reference (current_map_ref.py) on the one-GPU run's exported X -- X does not depend on the
sharding -- and the rank's own potentials.  (File name: sorts before the other GPU tests, see test_dist_sharded.py.)"""
import os
import queue
import socket
import traceback

import numpy as np
import pytest
import torch.multiprocessing as mp

import current_map_ref as cmr

pytestmark = pytest.mark.gpu

Vd = 5.0


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _solve(with_X):
    """charge -> potential -> power with the switch on, on a fresh state of the 2.5 nm device"""
    from devicekmc_amd import host, lib, params, structure
    L = lib.load()
    g = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    s = structure.load_structure(os.path.join(g, "device_2.5nm.npz"))
    p = params.KMCParameters(); p.solve_heating_global = True; p.cg_tol = 1e-10
    dev = host.Device(s, p); gb = dev.make_gpubuf("cuda:0")
    dev.setLaplacePotential(gb, p, Vd); gb.sync_HostToGPU(dev)
    dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, 0)
    L.dkmc_set_current_map(1)
    try:
        dev.updatePower(gb, p, Vd)
    finally:
        L.dkmc_set_current_map(0)
    out = dict(map=(dev.site_current, dev.site_current_tunnel, dev.site_tunnel_outflow), info=[dev.current_map_info[k] for k in dev.CURRENT_MAP_INFO],
               imacro=dev.imacro, m=gb.t["atom_virtual_potentials"].cpu().numpy().copy(), stats=dict(host.get_stats()))
    if with_X:
        out.update(X=host.get_last_X(), atoms=[gb.t[n].cpu().numpy().copy() for n in ("atom_x", "atom_y", "atom_z")],
                   site_element=gb.t["site_element"].cpu().numpy().copy(), N=dev.N, nn_dist=p.nn_dist, lattice=p.lattice, pbc=int(p.pbc))
    return out


def _worker(rank, world, port, q):
    try:
        os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        import torch
        from devicekmc_amd import parallel
        parallel.init("gloo")
        torch.cuda.set_device(0)
        one = _solve(True) if rank == 0 else None             # single-GPU path, no communicator
        parallel.barrier()
        assert parallel.attach_solver_comm() == "host"
        got = _solve(False)
        parallel.detach_solver_comm()
        parallel.barrier()
        q.put((rank, None, one, got))
        parallel.finalize()
    except Exception:
        q.put((rank, traceback.format_exc(), None, None))
        raise


def test_two_ranks_end_with_the_same_map():
    import __graft_entry__ as g
    g.build()
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs: p.start()
    out = []
    try:
        for _ in range(world):
            out.append(q.get(timeout=300))
            assert out[-1][1] is None, out[-1][1]             # a rank failed: the test ends here
        for p in procs:
            p.join(60); assert p.exitcode == 0, p.exitcode
    except (queue.Empty, AssertionError):
        for p in procs:
            if p.is_alive(): p.kill()
        for p in procs: p.join(10)
        raise
    (_, _, one, g0), (_, _, _, g1) = sorted(out, key=lambda t: t[0])
    assert g0["stats"]["comm_ranks"] == 2 and g0["stats"]["xt_ns"] > 0
    assert g0["stats"]["xt_local_subblocks"] + g1["stats"]["xt_local_subblocks"] == g0["stats"]["xt_subblocks"] > 0
    for a, b in zip(g0["map"], g1["map"]):
        assert a.tobytes() == b.tobytes()
    assert np.array(g0["info"]).tobytes() == np.array(g1["info"]).tobytes() and g0["info"][6] == 2
    ax, ay, az = one["atoms"]
    for got in (one, g0, g1):
        ref = cmr.reference(one["X"], got["m"], ax, ay, az, cmr.atom_sites(one["site_element"]), one["N"], one["nn_dist"], one["lattice"], one["pbc"])
        cmr.check(got["map"], got["info"], ref, got["imacro"])
        assert ref["thr_tun"].max() > 0
