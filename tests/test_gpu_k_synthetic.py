"""K -- patterns, charge rule, the form the solve runs on, assembly, one product and the converged K-CG -- against the longdouble host reference
(tests/k_ref.py, pinned by tests/test_k_ref.py) on the synthetic lattice devices of tests/k_cases.py, whose rows have 1 ... 85 off-diagonals:
every width at which the CSR product takes another pass and the blocked form another row width, the refusal above 64, rows linked to both
contacts, every branch of the three link rules, contact boundaries inside a layer, and (case L, 135 210 rows) more rows than one grid of any
vector kernel and three passes of a block of the blocked form.  Every comparison is with the reference, none with the CPU oracle.

Through the C ABI: dkmc_initialize_sparsity (host.Device.make_gpubuf), dkmc_update_charge_gpu, dkmc_background_potential_gpu_sparse,
dkmc_update_CB_edge_gpu_sparse and the test aid dkmc_debug_k_system, on both forms small systems reach (dkmc_set_k_blocked).

Bounds.  u = 2^-53.  A sum of n float64 terms formed in any order lies within (n - 1) u sum|terms| of the exact sum: the assembled diagonal and
right-hand side pass within (n + 2) u sum|terms| of the longdouble values (n: links of the row), a product row within (n + 3) u sum_j |k_ij v_j|
(n: its device links and the diagonal).
A solve passes when the longdouble || D^-1/2 (K_ref y - b_ref) ||_2 of the field it leaves is at most 10 tol (the factor of the K and heat tests).
Every check prints "k-pin <check> <case>: worst / bound" for DESIGN.md section 2."""
import ctypes as C

import numpy as np
import pytest

import k_cases
import k_ref
from test_gpu_parity import _d2h_i32, get, hip, put  # noqa: F401

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
Q = 1.60217663e-19
FORMS = (1, 0)                       # dkmc_set_k_blocked when the pattern is built
_cases, _devs = {}, {}


@pytest.fixture(autouse=True)
def _switches(hip):
    host, L = hip
    yield
    L.dkmc_set_k_blocked(1); L.dkmc_set_cb_edge_domain(0); L.dkmc_set_cg_tolerance(1e-6)


def _note(check, name, worst, bound=1.0):
    print("k-pin %-26s %-12s: %.3e / %.3e" % (check, name, worst, bound))


def _ratio(err, bound):
    """worst err / bound; where the bound is zero the values must agree exactly"""
    err, bound = np.atleast_1d(err), np.atleast_1d(bound)
    assert not np.isnan(err.astype(np.float64)).any()
    assert np.all(err[bound == 0] == 0)
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def _case(name):
    """structure, parameters, neighbour index and reference charges of a case; systems and solutions are added as they are asked for"""
    if name not in _cases:
        from oracle import oracle as oc
        s, p = k_cases.make_case(name)
        neigh, nn = oc.build_neighbors(s.x, s.y, s.z, np.asarray(p.lattice, dtype=np.float64), p.pbc, p.nn_dist)
        charge = k_ref.charges(neigh, s.element, np.zeros(len(s.element), dtype=np.int32), p.metals)
        _cases[name] = dict(name=name, s=s, p=p, neigh=np.asarray(neigh), charge=charge, N=len(s.element), n=p.num_atoms_first_layer, sys={}, sol={})
    return _cases[name]


def _system(c, rule, Vd):
    if (rule, Vd) not in c["sys"]:
        c["sys"][rule, Vd] = k_cases.reference_of(k_ref, c["p"], c["neigh"], c["s"].element, c["charge"], Vd, rule)
    return c["sys"][rule, Vd]


def _solution(c, rule, Vd):
    if (rule, Vd) not in c["sol"]:
        c["sol"][rule, Vd] = k_ref.solve(_system(c, rule, Vd))[0]
    return c["sol"][rule, Vd]


def _device(c, hip, blocked):
    """(Device, GPUBuffers) of a case with its pattern built under dkmc_set_k_blocked(blocked) and the charges updated, kept for the module.
    Case L takes its neighbour index from the GPU builder; every index is asserted equal to the one the reference is built from."""
    host, L = hip
    key = (c["name"], blocked)
    if key not in _devs:
        L.dkmc_set_k_blocked(blocked)
        try:
            dev = host.Device(c["s"], c["p"], gpu_neighbors="cuda:0" if c["name"] == "L" else None)
            assert np.array_equal(dev.neigh_idx, c["neigh"])
            gb = dev.make_gpubuf("cuda:0")
        finally:
            L.dkmc_set_k_blocked(1)
        dev.updateCharge(gb)
        _devs[key] = (dev, gb)
    return _devs[key]


def _form_info(L, gb):
    from devicekmc_amd.lib import check
    info = (C.c_longlong * 9)()
    check(L.dkmc_kcg_form_info(C.byref(gb.c), info))
    return list(info)


def _contacts(rule, Vd):
    return (-Vd / 2, Vd / 2) if rule == 0 else (Vd / 2, -Vd / 2)


def _solve(hip, c, gb, rule, Vd, tol, start=None):
    """one solve through the C ABI from `start` (volts, all sites; default zeros).  Returns (field as left in the buffer, iterations, r.r, form used)"""
    from devicekmc_amd.lib import check
    host, L = hip
    p, N, n = c["p"], c["N"], c["n"]
    field = "site_potential_boundary" if rule == 0 else "site_CB_edge"
    put(gb, field, np.zeros(N) if start is None else start)
    L.dkmc_set_cg_tolerance(tol)
    try:
        if rule == 0:
            check(L.dkmc_background_potential_gpu_sparse(C.byref(gb.c), N, n, n, Vd, int(p.pbc), p.high_G, p.low_G, p.nn_dist, len(p.metals), 0))
        else:
            L.dkmc_set_cb_edge_domain(1 if rule == 2 else 0)
            check(L.dkmc_update_CB_edge_gpu_sparse(C.byref(gb.c), N, n, n, Vd, int(p.pbc), p.high_G, p.low_G, p.nn_dist, len(p.metals)))
    finally:
        L.dkmc_set_cb_edge_domain(0); L.dkmc_set_cg_tolerance(1e-6)
    st = host.get_stats()
    it, rr = (st["cg_iters_K"], st["cg_rr_K"]) if rule == 0 else (st["cg_iters_CB"], st["cg_rr_CB"])
    return get(gb, field).copy(), it, rr, st["kcg_blocked"]


def _check_solve(c, rule, Vd, tol, out, it, rr, label):
    """contacts re-imposed exactly, r.r of the loop at most tol^2, the reference residual of the rows at most 10 tol; returns the rows in volts"""
    N, n = c["N"], c["n"]
    S = _system(c, rule, Vd)
    VL, VR = _contacts(rule, Vd)
    scale = 1.0 if rule == 0 else Q
    assert np.all(out[:n] == VL * scale) and np.all(out[N - n:] == VR * scale), label
    y = out[n:N - n] / scale
    assert np.isfinite(y).all(), label
    res = k_ref.scaled_residual(S, y)
    _note("solve residual / 10 tol", label, res, 10 * tol)
    assert res <= 10 * tol, label
    assert rr <= tol * tol, (label, rr)
    if Vd != 0.0:
        assert it > 0, label
    if rule == 2:
        assert np.all(out[n:N - n][S["identity"]] == 0.0), label
    return y


def _system_export(hip, c, gb, rule, Vd, v):
    from devicekmc_amd.lib import check
    host, L = hip
    p, N, n = c["p"], c["N"], c["n"]
    m = N - 2 * n
    VL, VR = _contacts(rule, Vd)
    v = np.ascontiguousarray(v, dtype=np.float64)
    t, d, b = np.zeros(m), np.zeros(m), np.zeros(m)
    check(L.dkmc_debug_k_system(C.byref(gb.c), rule, N, n, n, VL, VR, p.high_G, p.low_G, len(p.metals), v.ctypes.data, t.ctypes.data, d.ctypes.data, b.ctypes.data))
    return t, d, b


# ---- patterns, charges, form ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", k_cases.SMALL + ["L"])
def test_patterns_charges_and_form(name, hip):
    host, L = hip
    c = _case(name)
    (P, Pl, Pr), _ = k_ref.patterns(c["neigh"], c["n"])
    m = c["N"] - 2 * c["n"]
    od = np.diff(P[0]) - 1
    R = (-(-m // 256) + 63) // 64 * 64
    for blocked in FORMS:
        dev, gb = _device(c, hip, blocked)
        assert np.array_equal(get(gb, "site_charge"), c["charge"]), name
        g = gb.c
        for (rp_name, ci_name, nnz_name), (rp, ci) in zip((("Device_row_ptr_d", "Device_col_indices_d", "Device_nnz"),
                                                           ("contact_left_row_ptr", "contact_left_col_indices", "contact_left_nnz"),
                                                           ("contact_right_row_ptr", "contact_right_col_indices", "contact_right_nnz")), (P, Pl, Pr)):
            nnz = getattr(g, nnz_name)
            assert nnz == len(ci) == rp[m], (name, rp_name)
            assert np.array_equal(_d2h_i32(getattr(g, rp_name), m + 1), rp), (name, rp_name)
            if nnz:
                assert np.array_equal(_d2h_i32(getattr(g, ci_name), nnz), ci), (name, ci_name)
        info = _form_info(L, gb)
        if blocked and k_cases.BLOCKED[name]:
            total = 64 * int((od > 32).sum()) + 32 * int((od <= 32).sum())
            assert info[:4] == [1, m, R, -(-m // R)] and info[8] == total, (name, info)
        else:
            assert info == [0] * 9, (name, info)
        _, it, rr, used = _solve(hip, c, gb, 0, 5.0, 1e-10)
        assert used == (1 if blocked and k_cases.BLOCKED[name] else 0), name
    if name == "d":
        assert (od > 64).any()
    if name == "L":
        assert R == 576 and m > 131072


# ---- assembly and one product, through the export ------------------------------------------------------------------------------------------------------
def _probe_vectors(S):
    """a fixed-seed normal vector, ones, and a unit vector for a row of each width class that exists (<= 32, 33 ... 64, > 64 off-diagonals)"""
    m, od = S["m"], S["offdiag"]
    vs = [("normal", np.random.default_rng(5).standard_normal(m)), ("ones", np.ones(m))]
    for label, sel in (("e_narrow", od <= 32), ("e_wide", (od > 32) & (od <= 64)), ("e_over", od > 64)):
        k = np.flatnonzero(sel)
        if len(k):
            e = np.zeros(m); e[k[len(k) // 2]] = 1.0
            vs.append((label, e))
    return vs


@pytest.mark.parametrize("rule", [0, 1, 2])
@pytest.mark.parametrize("name", k_cases.SMALL + ["L"])
def test_assembly_and_product_against_the_reference(name, rule, hip):
    c = _case(name)
    for Vd in k_cases.biases(name):
        S = _system(c, rule, Vd)
        label = "%s/r%d/%+g" % (name, rule, Vd)
        kept = {}
        for blocked in FORMS:
            dev, gb = _device(c, hip, blocked)
            form = "blocked" if blocked and k_cases.BLOCKED[name] else "csr"
            for vi, (vname, v) in enumerate(_probe_vectors(S)):
                t, d, b = _system_export(hip, c, gb, rule, Vd, v)
                if vi == 0:
                    wd = _ratio(np.abs(d.astype(LD) - S["diag"]), (S["nterm"] + 2) * U * np.where(S["identity"], 0, S["diag"]))
                    wb = _ratio(np.abs(b.astype(LD) - S["rhs"]), (S["nrhs"] + 2) * U * S["rhs_abs"])
                    _note("diagonal %s" % form, label, wd); _note("rhs %s" % form, label, wb)
                    assert wd <= 1 and wb <= 1, label
                    if rule == 2:
                        assert S["identity"].any() and np.all(d[S["identity"]] == 1.0) and np.all(b[S["identity"]] == 0.0), label
                bound = (S["nprod"] + 3) * U * k_ref.product(S, v, absolute=True)
                err = np.abs(t.astype(LD) - k_ref.product(S, v))
                w = _ratio(err, bound)
                _note("product %s %s" % (form, vname), label, w)
                assert w <= 1, (label, vname)
                if vname in kept:
                    w2 = _ratio(np.abs(t - kept[vname]).astype(LD), 2 * bound)
                    _note("product blocked vs csr %s" % vname, label, w2)
                    assert w2 <= 1, (label, vname)
                kept[vname] = t


# ---- the solves --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", [0, 1, 2])
@pytest.mark.parametrize("name", k_cases.SMALL)
def test_solves_against_the_reference(name, rule, hip):
    c = _case(name)
    tols = (1e-10, 1e-12) if name in ("a", "c", "d") else (1e-10,)
    for Vd in k_cases.biases(name):
        if Vd == 0.0:
            continue                                                    # test_zero_bias
        yref = _solution(c, rule, Vd)
        for blocked in FORMS:
            dev, gb = _device(c, hip, blocked)
            for tol in tols:
                label = "%s/r%d/%+g/%s/%g" % (name, rule, Vd, "blocked" if blocked and k_cases.BLOCKED[name] else "csr", tol)
                out, it, rr, used = _solve(hip, c, gb, rule, Vd, tol)
                assert used == (1 if blocked and k_cases.BLOCKED[name] else 0), label
                y = _check_solve(c, rule, Vd, tol, out, it, rr, label)
                print("k-pin max |y - y_ref| [V]        %-12s: %.3e after %d iterations" % (label, float(np.abs(y.astype(LD) - yref).max()), it))


@pytest.mark.parametrize("rule", [0, 1, 2])
def test_large_case_solves(rule, hip):
    """Case L: 135 210 rows, R = 576 (blocked: passes of 256, 256 and 64 rows; k_kc_step wraps its grid), CSR: k_kc_apply, k_kc_update and
    k_kc_direction wrap theirs.  The residual only: no LU of this size on a test machine."""
    c = _case("L")
    for blocked in FORMS:
        dev, gb = _device(c, hip, blocked)
        label = "L/r%d/%s" % (rule, "blocked" if blocked else "csr")
        out, it, rr, used = _solve(hip, c, gb, rule, 5.0, 1e-10)
        assert used == blocked, label
        _check_solve(c, rule, 5.0, 1e-10, out, it, rr, label)
        print("k-pin iterations                 %-12s: %d" % (label, it))


# ---- edges ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", [0, 1, 2])
def test_zero_bias(rule, hip):
    c = _case("a")
    for blocked in FORMS:
        dev, gb = _device(c, hip, blocked)
        out, it, rr, used = _solve(hip, c, gb, rule, 0.0, 1e-10)
        assert it == 0 and rr == 0.0 and not np.isnan(out).any() and not out.any(), (rule, blocked, it, rr)


@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("name", ["a", "d"])
def test_second_solve_from_the_converged_field(name, rule, hip):
    c = _case(name)
    tol = 1e-10
    for blocked in FORMS:
        dev, gb = _device(c, hip, blocked)
        label = "%s/r%d/%s/again" % (name, rule, "blocked" if blocked and k_cases.BLOCKED[name] else "csr")
        out, it, rr, _ = _solve(hip, c, gb, rule, 5.0, tol)
        _check_solve(c, rule, 5.0, tol, out, it, rr, label)
        out2, it2, rr2, _ = _solve(hip, c, gb, rule, 5.0, tol, start=out if rule == 0 else out / Q)
        S = _system(c, rule, 5.0)
        n, N = c["n"], c["N"]
        res = k_ref.scaled_residual(S, out2[n:N - n] / (1.0 if rule == 0 else Q))
        _note("solve residual / 10 tol", label, res, 10 * tol)
        assert res <= 10 * tol and rr2 <= tol * tol and it2 < it, (label, it, it2)


def test_pattern_rebuilt_for_other_contacts_refuses_the_old_ones(hip):
    host, L = hip
    c = _case("a")
    p, N, n = c["p"], c["N"], c["n"]
    dev = host.Device(c["s"], p)
    gb = dev.make_gpubuf("cuda:0")
    dev.updateCharge(gb)
    args = (int(p.pbc), p.high_G, p.low_G, p.nn_dist, len(p.metals), 0)
    assert L.dkmc_background_potential_gpu_sparse(C.byref(gb.c), N, n, n, 5.0, *args) == 0
    assert L.dkmc_initialize_sparsity(C.byref(gb.c), int(p.pbc), p.nn_dist, n + 1) == 0
    assert L.dkmc_background_potential_gpu_sparse(C.byref(gb.c), N, n, n, 5.0, *args) == 6
    assert b"contact sizes" in L.dkmc_last_error()
    v = np.zeros(N - 2 * n); o = [np.zeros(N - 2 * n) for _ in range(3)]
    assert L.dkmc_debug_k_system(C.byref(gb.c), 0, N, n, n, -2.5, 2.5, p.high_G, p.low_G, len(p.metals), v.ctypes.data, *[a.ctypes.data for a in o]) == 6
    L.dkmc_clear_error()
    assert L.dkmc_background_potential_gpu_sparse(C.byref(gb.c), N, n + 1, n + 1, 5.0, *args) == 0


def test_two_buffers_keep_their_own_form(hip):
    host, L = hip
    a, cc = _case("a"), _case("c")
    (_, ga), (_, gc1), (_, gc0) = _device(a, hip, 1), _device(cc, hip, 1), _device(cc, hip, 0)
    before = [_form_info(L, g) for g in (ga, gc1, gc0)]
    assert before[0][:2] == [1, a["N"] - 2 * a["n"]] and before[1][:2] == [1, cc["N"] - 2 * cc["n"]] and before[2] == [0] * 9
    first = {}
    for rnd in range(2):
        for key, c, gb, form in (("a", a, ga, 1), ("c1", cc, gc1, 1), ("c0", cc, gc0, 0)):
            out, it, rr, used = _solve(hip, c, gb, 0, 5.0, 1e-10)
            assert used == form, (key, rnd)
            _check_solve(c, 0, 5.0, 1e-10, out, it, rr, "two buffers %s" % key)
            if rnd == 0:
                first[key] = (out, it)
            else:
                assert np.array_equal(out, first[key][0]) and it == first[key][1], key
    assert [_form_info(L, g) for g in (ga, gc1, gc0)] == before
