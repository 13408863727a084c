#!/usr/bin/env python3
"""Bits of the K solves on every form of csrc/kcg.hip, with whichever library is in place: one line per case, to be compared between two library
builds (cp tools/ab/lib_x.so devicekmc_amd/libdevicekmc_hip.so; python tools/ab/kcg_bits.py > x.txt; the same with the other; diff).
Every case: cg_tol 1e-10, CB edge (setLaplacePotential) and background potential (updatePotential) from the Laplace start; printed are the form the
solve used (stats kcg_blocked), cg_iters_K / cg_iters_CB, cg_rr_K / cg_rr_CB as hex floats, sha256 of site_potential_boundary and of site_CB_edge.
  2.5nm    blocked form and CSR positions (dkmc_set_k_blocked 1 / 0) x CB edge on sites / on atoms: CB = 0, 1, 2 of k_kb_assemble and k_kc_assemble
  7.5nm    (85 071 sites: blocks with 64-wide and 32-wide rows) the same two forms; the slab emulation (dkmc_kcg_emulate_slabs) with 1, 2, 5 virtual ranks
  tile:6   (338 364 sites, the smallest tile:K above 262 144 rows) dkmc_set_k_blocked_large(1): form 2 (dkmc_kcg_form_info), both solves, with 4-byte and
           with 2-byte stored words (dkmc_set_k_window_word_bytes): the two lines differ in `words` alone
usage: python tools/ab/kcg_bits.py [2.5nm 7.5nm tile:6]"""
import ctypes as C
import hashlib
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

Vd = 5.0


def sha(a):
    return hashlib.sha256(a.tobytes()).hexdigest()[:32]


def solve(name, blocked, domain, large=0, slabs=(), word_bytes=4):
    import torch
    from bench import make_workload
    from devicekmc_amd import host, lib
    L = lib.load()
    L.dkmc_set_k_blocked(blocked); L.dkmc_set_k_blocked_large(large)
    L.dkmc_set_k_window_word_bytes(word_bytes)
    try:
        s, p = make_workload(name)
        p.cg_tol = 1e-10; p.cb_edge_domain = domain
        dev = host.Device(s, p, gpu_neighbors="cuda:0") if name.startswith("tile:") else host.Device(s, p)
        gb = dev.make_gpubuf("cuda:0")
        info = (C.c_longlong * 9)()
        lib.check(L.dkmc_kcg_form_info(C.byref(gb.c), info))
        dev.setLaplacePotential(gb, p, Vd)
        st = host.get_stats()
        form_cb, it_cb, rr_cb = int(st["kcg_blocked"]), int(st["cg_iters_CB"]), float(st["cg_rr_CB"])
        cb = gb.site_CB_edge.cpu().numpy().copy()
        gb.sync_HostToGPU(dev)
        dev.updateCharge(gb)
        for nr in slabs:
            n1 = p.num_atoms_first_layer
            md, it_s, it_r = C.c_double(-1), C.c_int(0), C.c_int(0)
            us, hr = (C.c_double * 4)(), (C.c_longlong * 2)()
            lib.check(L.dkmc_kcg_emulate_slabs(C.byref(gb.c), dev.N, n1, n1, Vd, p.high_G, p.low_G, len(p.metals), nr, -1, 0,
                                               C.byref(md), C.byref(it_s), C.byref(it_r), us, hr))
            print("%s slabs N=%d iters_slab %d iters_one_gpu %d max_abs_diff %s halo %d largest_slab %d"
                  % (name, nr, it_s.value, it_r.value, float(md.value).hex(), hr[0], hr[1]), flush=True)
        dev.updatePotential(gb, p, Vd, 0)
        torch.cuda.synchronize()
        st = host.get_stats()
        print("%s k_blocked=%d large=%d words=%d cb_domain=%s form_info %d form_K %d form_CB %d iters_K %d iters_CB %d rr_K %s rr_CB %s phi %s cb_edge %s"
              % (name, blocked, large, word_bytes, domain, info[0], int(st["kcg_blocked"]), form_cb, int(st["cg_iters_K"]), it_cb, float(st["cg_rr_K"]).hex(), rr_cb.hex(),
                 sha(gb.site_potential_boundary.cpu().numpy()), sha(cb)), flush=True)
        del gb, dev
        torch.cuda.empty_cache()
    finally:
        L.dkmc_set_k_blocked(1); L.dkmc_set_k_blocked_large(0); L.dkmc_set_cb_edge_domain(0); L.dkmc_set_cg_tolerance(1e-6); L.dkmc_set_k_window_word_bytes(4)


def main():
    names = sys.argv[1:] or ["2.5nm", "7.5nm", "tile:6"]
    for name in names:
        if name == "2.5nm":
            for blocked in (1, 0):
                for domain in ("sites", "atoms"):
                    solve(name, blocked, domain)
        elif name == "7.5nm":
            solve(name, 1, "sites")
            solve(name, 0, "sites", slabs=(1, 2, 5))
        else:
            for domain in ("sites", "atoms"):
                solve(name, 1, domain, large=1)
                solve(name, 1, domain, large=1, word_bytes=2)


if __name__ == "__main__":
    main()
