"""16-bit stored words of the windowed blocked form of the CG on K (dkmc_set_k_window_word_bytes(2), csrc/kcg.hip k_kbw_apply<MODE, 2> + csrc/kbw_plan.h
kbw_halfword_pos) against its 4-byte words.  The two layouts hold the same plan, and every element of the product is the same sequence of fp64
operations -- the same entries in the same slots of the same lanes, the same pairwise sums --, so here, unlike between two FORMS of K (different
summation orders: converged solves or true residuals, never bits), the solves must agree bit for bit: iterates, iteration counts, r.r and everything
that follows from the potentials.  Workload: tile:6 (338 364 sites), the smallest tile:K above 262 144 rows, current off: blocks with 64-wide and
32-wide rows, blocks that turn a strip end, a short last block.  Every switch is read when a pattern is built: set before the device is built,
restored in a `finally`."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_kcg_windows import Vd, _form, _fresh, _oracle_K, _scaled_res

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__ as g
    g.build()
    from devicekmc_amd import host, lib
    return host, lib.load()


def _words(L, gb):
    from devicekmc_amd import lib
    info = (C.c_longlong * 3)()
    lib.check(L.dkmc_kcg_form_words(C.byref(gb.c), info))
    return list(info)


def _restore(L):
    L.dkmc_set_k_window_word_bytes(4); L.dkmc_set_k_blocked_large(0); L.dkmc_debug_kbw_segment_cap(0); L.dkmc_set_cg_tolerance(1e-6)


@pytest.fixture(scope="module")
def converged(hip):
    """CB edge (setLaplacePotential) and background potential (updatePotential) of tile:6 from the Laplace start at cg_tol = 1e-10, one build of the
    pattern per configuration: windowed form with 4-byte and with 2-byte words, switch off (CSR positions), 2-byte words with the segment cap forced to
    1 (the builder refuses: CSR positions)."""
    import torch
    host, L = hip
    out = {}
    try:
        for mode, large, wb, cap in (("w4", 1, 4, 0), ("w2", 1, 2, 0), ("off", 0, 4, 0), ("refused2", 1, 2, 1)):
            L.dkmc_set_k_blocked_large(large); L.dkmc_set_k_window_word_bytes(wb); L.dkmc_debug_kbw_segment_cap(cap)
            assert L.dkmc_get_k_window_word_bytes() == wb
            s, p, dev, sim, gb = _fresh("tile:6", cg_tol=1e-10)
            st = host.get_stats()
            rec = dict(form=_form(L, gb), words=_words(L, gb), kcg_cb=st["kcg_blocked"], iters_cb=st["cg_iters_CB"], rr_cb=st["cg_rr_CB"],
                       cb=gb.site_CB_edge.cpu().numpy().copy())
            dev.updateCharge(gb)
            dev.updatePotential(gb, p, Vd, 0)
            torch.cuda.synchronize()
            st = host.get_stats()
            rec.update(kcg=st["kcg_blocked"], iters=st["cg_iters_K"], rr=st["cg_rr_K"], bytes=st["kcg_bytes"],
                       phi=gb.site_potential_boundary.cpu().numpy().copy(), tol=p.cg_tol, nl=p.num_atoms_first_layer, N=s.N)
            if mode == "w2":
                K, rhs, nl, m = _oracle_K(s, p, dev, gb)
                rec["sres"] = _scaled_res(K, rhs, rec["phi"][nl:nl + m])
            out[mode] = rec
            del dev, sim, gb
            torch.cuda.empty_cache()
    finally:
        _restore(L)
    return out


@pytest.fixture(scope="module")
def supersteps(hip):
    """Three coupled supersteps of tile:6 (current off) at the library's default tolerance on the windowed form.  "w4": the word-bytes switch is left
    alone (the default); "w2": 2-byte words."""
    import torch
    host, L = hip
    out = {}
    try:
        for mode in ("w4", "w2"):
            L.dkmc_set_k_blocked_large(1)
            if mode == "w2":
                L.dkmc_set_k_window_word_bytes(2)
            s, p, dev, sim, gb = _fresh("tile:6")
            assert p.cg_tol == 1e-6
            rec = dict(words=_words(L, gb), getter=L.dkmc_get_k_window_word_bytes(), steps=[])
            for k in range(3):
                dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, k)
                torch.cuda.synchronize()
                st = host.get_stats()
                step = dict(kcg=st["kcg_blocked"], iters=st["cg_iters_K"], rr=st["cg_rr_K"],
                            pb=gb.site_potential_boundary.cpu().numpy().copy(), pc=gb.site_potential_charge.cpu().numpy().copy())
                _, dt = sim.executeKMCStep(gb, dev, want_log=True)
                step.update(log=np.array(sim.last_event_log).copy(), dt=dt, element=gb.site_element.cpu().numpy().copy(),
                            charge=gb.site_charge.cpu().numpy().copy())
                rec["steps"].append(step)
            out[mode] = rec
            del dev, sim, gb
            torch.cuda.empty_cache()
    finally:
        _restore(L)
    return out


def test_same_bits_as_the_4_byte_form(converged):
    """Both solves from the Laplace start at 1e-10: the same potentials bit for bit, the same iteration counts, the same r.r."""
    a, b = converged["w4"], converged["w2"]
    assert a["words"][0] == 4 and b["words"][0] == 2
    assert a["kcg"] == 2 and b["kcg"] == 2 and a["kcg_cb"] == 2 and b["kcg_cb"] == 2
    assert a["iters"] > 0 and a["iters_cb"] > 0
    assert np.array_equal(a["phi"], b["phi"])
    assert np.array_equal(a["cb"], b["cb"])
    assert (a["iters"], a["iters_cb"]) == (b["iters"], b["iters_cb"])
    assert a["rr"] == b["rr"] and a["rr_cb"] == b["rr_cb"]


def test_true_residual_of_the_2_byte_solution(converged):
    """The 2-byte solution meets the stop test in the TRUE scaled residual of the oracle's K (test_tile10_converged_agreement's bound)."""
    b = converged["w2"]
    print("tile:6, 2-byte words: scaled residual on the oracle's K %.3e (tol %.0e), r.r %.3e" % (b["sres"], b["tol"], b["rr"]))
    assert b["rr"] <= b["tol"] ** 2
    assert b["sres"] <= 10 * b["tol"], b["sres"]
    nl = b["nl"]
    assert (b["phi"][:nl] == -Vd / 2).all() and (b["phi"][-nl:] == Vd / 2).all()


def test_same_plan_half_the_word_bytes(converged):
    a, b = converged["w4"], converged["w2"]
    assert a["form"] == b["form"] and a["form"][0] == 2
    words = a["form"][8]
    assert words > 0 and a["words"] == [4, words, 4 * words] and b["words"] == [2, words, 2 * words]
    assert a["bytes"] - b["bytes"] == 2 * words


def test_coupled_supersteps_same_bits(supersteps):
    """Three supersteps at the default tolerance: identical event logs, dt, elements, charges and both potentials."""
    a, b = supersteps["w4"], supersteps["w2"]
    assert a["words"][0] == 4 and b["words"][0] == 2
    for k, (x, y) in enumerate(zip(a["steps"], b["steps"])):
        assert x["kcg"] == 2 and y["kcg"] == 2, k
        assert x["iters"] == y["iters"] and x["rr"] == y["rr"], k
        assert np.array_equal(x["pb"], y["pb"]) and np.array_equal(x["pc"], y["pc"]), k
        assert len(x["log"]) > 0 and np.array_equal(x["log"], y["log"]), k
        assert x["dt"] == y["dt"], k
        assert np.array_equal(x["element"], y["element"]) and np.array_equal(x["charge"], y["charge"]), k


def test_default_word_bytes_is_4(supersteps):
    a = supersteps["w4"]
    assert a["getter"] == 4 and a["words"][0] == 4


def test_refused_build_falls_back_to_csr_positions(converged):
    """2-byte words asked for, but the builder refuses (segment cap 1): CSR positions, bit for bit the switch-off run."""
    ref, off = converged["refused2"], converged["off"]
    assert ref["kcg"] == 0 and ref["form"][0] == 0 and ref["words"] == [0, 0, 0]
    assert off["kcg"] == 0 and off["words"] == [0, 0, 0]
    assert np.array_equal(ref["phi"], off["phi"]) and np.array_equal(ref["cb"], off["cb"])
    assert ref["bytes"] == off["bytes"]


def test_small_system_keeps_the_blocked_form(hip):
    """7.5 nm (85 071 sites, below 262 144 rows): form 1 whatever the word-bytes switch says; no windowed form, word bytes 0."""
    host, L = hip
    try:
        L.dkmc_set_k_blocked_large(1); L.dkmc_set_k_window_word_bytes(2)
        s, p, dev, sim, gb = _fresh("7.5nm")
        assert _form(L, gb)[0] == 1 and _words(L, gb)[0] == 0
        dev.updateCharge(gb); dev.updatePotential(gb, p, Vd, 0)
        assert host.get_stats()["kcg_blocked"] == 1
    finally:
        _restore(L)
