"""The sampled kernel profile of the three host loops that solve the current (dkmc_set_profiling(1); bench.py builds its roofline from it): how many
launches a solve samples follows from the loop's batch plan, the hint the previous solve left and the iterations the solve took -- restated here in
plain Python, not asked of the library -- and profiling changes nothing the solve computes.  2.5 nm device: the smallest with tiles, long rows and a
K system.  Both solves of a case start from zero (dkmc_set_current_warm_start(0) and a zeroed start vector), so that the second one iterates too."""
import numpy as np
import pytest

from test_gpu_parity import get, hip, put  # noqa: F401

pytestmark = pytest.mark.gpu
V = 5.0


def samples(first, later, iters):
    """Sampled launches that count in a solve of `iters` iterations: batches of `first`, then `later` (None: doubling up to 64) while fewer
    iterations are enqueued than the solve takes; positions 0, 8, ... 56 of a batch, if their iteration index is below `iters`."""
    n, it, batch = 0, 0, first
    while it < iters:
        n += sum(1 for b in range(0, min(batch, 64), 8) if it + b < iters)
        it += batch
        batch = later if later else (batch * 2 if batch < 64 else batch)
    return n


def block_plan(hint):                  # block-CG: three quarters of the previous solve's sweeps, then eights; no hint: 4, 8, ... 64
    return (max(4, 3 * hint // 4), 8) if hint > 12 else (4, None)


def vector_plan(hint):                 # single-vector CG, tiled or CSR: eight below the previous count, then eights; no hint: 8, 16, ... 64
    return (hint - 8, 8) if hint > 24 else (8, None)


CASES = {"block": (lambda L: (L.dkmc_set_x_block(16), L.dkmc_set_x_poly(0)), block_plan),
         "vector_tiled": (lambda L: L.dkmc_set_x_block(1), vector_plan),
         "vector_csr": (lambda L: L.dkmc_set_x_format(0), vector_plan)}


def two_solves(cell, hip, profile_second):
    """Two solves of the current on a fresh device; the stats and results of the two."""
    from devicekmc_amd import params as pm
    host, L = hip
    p = pm.KMCParameters(); p.solve_heating_global = False
    dev = host.Device(cell, p); gb = dev.make_gpubuf("cuda:0")
    dev.setLaplacePotential(gb, p, V); gb.sync_HostToGPU(dev)
    dev.updateCharge(gb); dev.updatePotential(gb, p, V, 0)
    out = []
    for k in range(2):
        L.dkmc_set_profiling(1 if (k == 1 and profile_second) else 0)
        put(gb, "atom_virtual_potentials", np.zeros(dev.N_atom + 2)); dev.updatePower(gb, p, V)
        out.append((host.get_stats(), dev.imacro, get(gb, "atom_virtual_potentials").copy()))
    return out


@pytest.mark.parametrize("case", sorted(CASES))
def test_sampled_profile_follows_the_plan_and_changes_nothing(cell_2p5, hip, case):
    host, L = hip
    switches, plan = CASES[case]
    try:
        L.dkmc_set_current_warm_start(0)
        switches(L)
        (st1, _, _), (st2, i2, m2) = two_solves(cell_2p5, hip, True)
        hint, iters = st1["cg_iters_X"], st2["cg_iters_X"]
        want = samples(*plan(hint), iters)
        print(case, "hint", hint, "iterations", iters, "samples", want, "long", st2["spmv_long_launches"], st2["spmv_long_ms"],
              "short", st2["spmv_short_launches"], st2["spmv_short_ms"])
        assert iters > 0 and want > 0
        if case == "block":
            assert st1["xb_fallback"] == 0 and st2["xb_fallback"] == 0 and st2["xb_width"] == 16
        assert st2["spmv_long_launches"] == want and st2["spmv_short_launches"] == want
        assert st2["spmv_long_ms"] > 0 and st2["spmv_short_ms"] > 0
        (_, _, _), (st3, i3, m3) = two_solves(cell_2p5, hip, False)
        assert st3["cg_iters_X"] == iters and st3["cg_rr_X"] == st2["cg_rr_X"]
        assert i3 == i2 and np.array_equal(m3, m2)
    finally:
        L.dkmc_set_profiling(0); L.dkmc_set_current_warm_start(1); L.dkmc_set_x_block(16); L.dkmc_set_x_format(1); L.dkmc_set_x_poly(8)
