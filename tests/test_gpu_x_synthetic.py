"""The tiled current-solve matrix X against the longdouble host reference (tests/x_ref.py, pinned by tests/test_x_ref.py) on the synthetic lattice
devices of tests/x_cases.py, whose |S| = ns and inner-contact metal count nM sit at 0, 1, 2, 29 ... 38, 255 ... 257, 511 ... 513, 639 and 768: every
size at which the 32-row blocks, the 256-column windows, the slack window of ns_pad, the partial-tile masks and the kept all-metal strips change
shape.  Every comparison is with the reference, none with another kernel of the library.

Through host.Device on the synthetic Structure: the CB edge is PUT (put(gb, "site_CB_edge", ...)), the charges come from dev.updateCharge and are
asserted equal to the oracle's, which the reference is built from.

Bounds.  R = x_cases.R_KIND is the CPU oracle's measured deviation from the reference per kind of entry (the conditioning of the float64 formula the
oracle and the kernels share); a tunnelling value passes within 8 R.  Direct, boundary and row-0/1 entries are equal bit for bit.  A sum of n terms
formed in any order lies within (n - 1) u sum|terms| of the exact sum, u = 2^-53; the bounds below add that to the 8 R of the terms.
Every check prints "x-pin <check> <case>: worst / bound" for DESIGN.md section 2."""
import ctypes as C

import numpy as np
import pytest

import power_ref as pr
import x_cases
import x_ref
from test_gpu_parity import _scaled_residual, get, hip, put  # noqa: F401

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
R = x_cases.R_KIND
KEPT, FIRST, METALS = 0, 1, 2              # info[6] of dkmc_get_x_static_info
THETAS = (1e-10, 1e-6, 1e-4)             # 1e-10 is the library's auto threshold; at (64, 2, 257) every sub-block is live there, so two more
_cache = {}


@pytest.fixture(autouse=True)
def _switches(hip):
    """the tests own the switches conftest does not know"""
    host, L = hip

    def reset():
        L.dkmc_set_x_static_tiles(2); L.dkmc_debug_x_static_verify(0); L.dkmc_set_x_tile_f32(1); L.dkmc_debug_set_x_static_gate(0)
        L.dkmc_set_x_tile_drop(0.0); L.dkmc_set_x_tile_drop_unit(0); L.dkmc_debug_poison_fold_cells(0); L.dkmc_set_x_poly_auto(1)
    reset(); L.dkmc_set_x_tile_drop_auto(0)
    yield
    reset(); L.dkmc_set_x_tile_drop_auto(1)


def _note(check, name, worst, bound=1.0):
    print("x-pin %-22s %-10s: %.3e / %.3e" % (check, name, worst, bound))


def _ratio(err, bound):
    """worst err / bound; where the bound is zero the values must agree exactly"""
    err, bound = np.atleast_1d(err), np.atleast_1d(bound)
    assert np.all(err[bound == 0] == 0)
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def _reference(s, p, cb):
    """the reference of a state: charges and neighbour index from the CPU oracle (asserted equal to the device's by _device)"""
    from oracle import oracle as oc
    o = oc.OracleKMC(s.element, s.x, s.y, s.z, p)
    o.CB_edge[:] = cb
    o.update_charge()
    ref = x_cases.reference_of(x_ref, s, p, cb, o.element, o.charge, o.neigh)
    c = dict(s=s, p=p, cb=cb, charge=o.charge.copy(), neigh=o.neigh.copy(), ref=ref)
    k = ref["kind"]
    c["Rv"] = np.where(k == 1, R[1], np.where(k == 2, R[2], 0.0))                       # per CSR entry
    c["X64"] = (ref["rp"].astype(np.int32), ref["ci"].astype(np.int32), ref["val"].astype(np.float64))
    pos = {0: np.arange(ref["ns"]), 1: np.searchsorted(ref["S_atom"], ref["S_metals_first"])}
    for order in (0, 1):
        ix = np.ix_(pos[order], pos[order])
        T, pred, kT = ref["T"][ix], ref["pred"][ix], ref["kindT"][ix]
        masks, up = x_ref.census(pred)
        c[order] = dict(S=ref["S_atom"][pos[order]], T=T, up=up, masks=masks, RT=np.where(kT == 1, R[1], R[2]) * np.abs(T))
    return c


def _case(name):
    if name not in _cache:
        s, p, Vd, cb, counts = x_cases.make_case(name)
        c = _reference(s, p, cb)
        c.update(name=name, Vd=Vd, counts=counts)
        assert (c["ref"]["nM"], c["ref"]["ns"]) == counts
        _cache[name] = c
    return _cache[name]


def _device(c, hip, element=None):
    """(Device, GPUBuffers) of a case with the CB edge put and the charges updated; element: another site_element than the structure's"""
    host, L = hip
    dev = host.Device(c["s"], c["p"])
    assert np.array_equal(dev.neigh_idx, c["neigh"])
    dev.site_CB_edge = c["cb"].copy()
    gb = dev.make_gpubuf("cuda:0")
    put(gb, "site_CB_edge", c["cb"])
    if element is not None:
        put(gb, "site_element", element)
    dev.updateCharge(gb)
    if element is None:
        assert np.array_equal(get(gb, "site_charge"), c["charge"])
    return dev, gb


def _tiles(L):
    from devicekmc_amd.lib import check
    nt, nsub = C.c_longlong(-1), C.c_longlong(-1)
    check(L.dkmc_xt_get_tiles(C.byref(nt), C.byref(nsub), None, None))
    tiles = np.zeros((nt.value, 4), dtype=np.int32); tval = np.zeros(nsub.value * 1024)
    if nt.value:
        check(L.dkmc_xt_get_tiles(None, None, tiles.ctypes.data, tval.ctypes.data))
    return tiles.astype(np.int64), tval.reshape(-1, 32, 32)


def _srow(L):
    from devicekmc_amd.lib import check
    n = C.c_int(-1)
    check(L.dkmc_xt_get_srow(C.byref(n), None))
    out = np.zeros(n.value, dtype=np.int32)
    check(L.dkmc_xt_get_srow(C.byref(n), out.ctypes.data))
    return out


def _static_info(L):
    from devicekmc_amd.lib import check
    a = (C.c_longlong * 8)(); v = (C.c_longlong * 4)()
    check(L.dkmc_get_x_static_info(a)); check(L.dkmc_debug_get_x_static_verify(v))
    return list(a), list(v)


def _live_info(L):
    from devicekmc_amd.lib import check
    a = (C.c_longlong * 8)()
    check(L.dkmc_get_x_tile_live_info(a, None))
    return list(a)


def _check_csr(c, X, label):
    """exported CSR against the reference: pattern exact; direct / boundary / row-0/1 entries bit for bit; tunnelling values within 8 R; the diagonal
    within sum 8 R |t| + n_i u sum|off| (n_i - 1 off-diagonals added in any order, one subtraction from the ground term)"""
    ref = c["ref"]
    rp, ci, data = X
    assert np.array_equal(rp, ref["rp"]) and np.array_equal(ci, ref["ci"]), label
    v, k = ref["val"], ref["kind"]
    exact = (k == 0) | (k == 3)
    assert np.array_equal(data[exact].astype(LD), v[exact]), label
    err = np.abs(data.astype(LD) - v)
    tun = (k == 1) | (k == 2)
    worst = _ratio(err[tun], 8 * c["Rv"][tun] * np.abs(v[tun])) if tun.any() else 0.0
    _note("csr values / 8R", label, worst)
    assert worst <= 1, label
    rowb = np.zeros(len(rp) - 1, dtype=LD); np.add.at(rowb, ref["row"], 8 * c["Rv"] * np.abs(v))
    dp = ref["diag_pos"]
    dworst = _ratio(err[dp], rowb + np.diff(rp) * U * ref["offabs"])
    _note("csr diagonal", label, dworst)
    assert dworst <= 1, label


def _check_store(c, order, L, label):
    """the tile store itself: S in the order in force, the tile list = the non-empty cells of the reference census (strip-major), equal masks, every
    stored element the reference's T or 0.0, and the diagonal pass = the row sums of T"""
    from devicekmc_amd.lib import check
    ref, o = c["ref"], c[order]
    ns = ref["ns"]
    assert np.array_equal(_srow(L), o["S"] + 2), label
    tiles, tval = _tiles(L)
    masks = o["masks"]
    want, soff = [], 0
    for w in range(masks.shape[1]):
        for k in range(masks.shape[0]):
            if masks[k, w]:
                want.append((k, w, masks[k, w], soff)); soff += bin(int(masks[k, w])).count("1")
    want = np.array(want, dtype=np.int64).reshape(-1, 4)
    assert np.array_equal(tiles, want), label
    assert len(tval) == soff, label
    worst = 0.0
    for k, w, mask, so in want:
        sl = 0
        for q in range(8):
            if not (mask >> q) & 1:
                continue
            got = tval[so + sl].astype(LD); sl += 1
            exp = x_ref.tile_values(o["T"], o["up"], k, w, q)
            r0, c0 = 32 * k, 256 * w + 32 * q
            bnd = np.zeros((32, 32), dtype=LD)
            r1, c1 = min(r0 + 32, ns), min(c0 + 32, ns)
            if r1 > r0 and c1 > c0:
                bnd[:r1 - r0, :c1 - c0] = 8 * np.where(o["up"][r0:r1, c0:c1], o["RT"][r0:r1, c0:c1], 0)
            assert np.array_equal(got[exp == 0], exp[exp == 0]), (label, k, w, q)      # 0.0 below the diagonal, beyond ns, where the pair fails
            worst = max(worst, _ratio(np.abs(got - exp), bnd))
    _note("tile values / 8R", label, worst)
    assert worst <= 1, label
    d = np.zeros(ref["Na"] + 1)
    check(L.dkmc_xt_get_diag(d.ctypes.data))
    rows = o["S"] + 2
    outside = np.ones(len(d), dtype=bool); outside[rows] = False
    assert np.all(d[outside] == 0.0), label
    if ns:
        exact = o["T"].sum(axis=1); mag = np.abs(o["T"]).sum(axis=1)
        dw = _ratio(np.abs(d[rows].astype(LD) - exact), 8 * o["RT"].sum(axis=1) + ns * U * mag)
        _note("tile diagonal pass", label, dw)
        assert dw <= 1, label


# ---- assembly, both storage forms ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("name", x_cases.NAMES)
def test_assembly_against_the_reference(name, fmt, hip):
    host, L = hip
    c = _case(name)
    L.dkmc_set_x_format(fmt)
    dev, gb = _device(c, hip)
    dev.updatePower(gb, c["p"], c["Vd"])
    st = host.get_stats()
    assert st["X_nnz"] == len(c["ref"]["ci"]) and st["N_atom"] == c["ref"]["Na"]
    if fmt:
        assert st["xt_ns"] == c["counts"][1]
    _check_csr(c, host.get_last_X(), "%s/%s" % (name, "tiled" if fmt else "csr"))


# ---- the tile store itself, both orders of S --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("name", x_cases.NAMES)
def test_tile_store_against_the_reference(name, order, hip):
    """order 0: dkmc_set_x_static_tiles(0), atom order.  order 1: the metals first, reached through mode 2 with its gate moved to ns (the rule takes
    the new order from the gate on) -- mode 1 is what the kept-strip tests below run."""
    host, L = hip
    c = _case(name)
    ns = c["counts"][1]
    if order:
        L.dkmc_set_x_static_tiles(2); L.dkmc_debug_set_x_static_gate(max(ns, 1))
    else:
        L.dkmc_set_x_static_tiles(0)
    dev, gb = _device(c, hip)
    dev.updatePower(gb, c["p"], c["Vd"])
    info, _ = _static_info(L)
    assert info[0] == (1 if order and ns >= 1 else 0), info
    assert host.get_stats()["xt_ns"] == ns
    _check_store(c, order, L, "%s/order%d" % (name, order))
    _check_csr(c, host.get_last_X(), "%s/order%d" % (name, order))


# ---- products ---------------------------------------------------------------------------------------------------------------------------------------------------
def _test_panel(ns):
    r = np.arange(ns, dtype=np.uint64)[:, None]; v = np.arange(16, dtype=np.uint64)[None, :]
    h = (((r * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) ^ (v * np.uint64(40503))) >> np.uint64(20)
    return 0.25 + h.astype(np.float64) / 4096.0 + 0.125 * v.astype(np.float64)


@pytest.mark.parametrize("name", x_cases.NAMES)
def test_products_against_the_reference(name, hip):
    """dkmc_xtb_tile_product at widths 16 and 4 against T V in longdouble on the documented test vectors, from the fp64 store and from the fp32 image
    (made by a solve at tolerance 1e-8: the assembly makes none below that); bound sum_j (8 R + (ns + 8) u) |t_ij v_j|, plus 2^-24 |t_ij v_j| per
    term from the image.  dkmc_xtb_check_product within its 1e-12, dkmc_xt_check_shares at 2, 3 and 8 virtual ranks."""
    from devicekmc_amd.lib import DeviceKMCError, check
    import copy
    host, L = hip
    c = _case(name)
    ns = c["counts"][1]
    p = copy.deepcopy(c["p"]); p.cg_tol = 1e-8
    dev, gb = _device(c, hip)
    dev.updatePower(gb, p, c["Vd"])
    st = host.get_stats()
    o = c[0]
    d, a = C.c_double(-1.0), C.c_double(-1.0)
    if ns == 0:
        with pytest.raises(DeviceKMCError):
            check(L.dkmc_xtb_tile_product(16, 8, np.zeros(16).ctypes.data))
        with pytest.raises(DeviceKMCError):
            check(L.dkmc_xtb_check_product(16, C.byref(d), C.byref(a)))
    else:
        V = _test_panel(ns).astype(LD)
        exact = o["T"] @ V; mag = np.abs(o["T"]) @ np.abs(V); rmag = o["RT"] @ np.abs(V)
        have_image = st["x_tile_f32_bytes"] > 0
        assert have_image == (st["spmv_tiles"] > 0)
        for width in (16, 4):
            for stored in (8, 4):
                out = np.zeros((ns, width))
                if stored == 4 and not have_image:
                    with pytest.raises(DeviceKMCError):
                        check(L.dkmc_xtb_tile_product(width, stored, out.ctypes.data))
                    continue
                check(L.dkmc_xtb_tile_product(width, stored, out.ctypes.data))
                bound = 8 * rmag[:, :width] + ((ns + 8) * U + (2.0 ** -24 if stored == 4 else 0.0)) * mag[:, :width]
                worst = _ratio(np.abs(out.astype(LD) - exact[:, :width]), bound)
                _note("product w%d fp%d" % (width, 8 * stored), name, worst)
                assert worst <= 1, (width, stored)
            check(L.dkmc_xtb_check_product(width, C.byref(d), C.byref(a)))
            _note("check_product w%d" % width, name, d.value, 1e-12 * a.value)
            assert d.value <= 1e-12 * a.value and (a.value > 0) == (st["spmv_tiles"] > 0)
    sb, its, itot = C.c_longlong(-1), C.c_longlong(-1), C.c_int(-1)
    for nr in (2, 3, 8):
        check(L.dkmc_xt_check_shares(nr, C.byref(d), C.byref(a), C.byref(sb), C.byref(its), C.byref(itot)))
        assert sb.value == st["xt_subblocks"] == len(_tiles(L)[1]) and its.value == itot.value, (nr, sb.value, its.value, itot.value)
        assert d.value <= 1e-12 * a.value and (a.value > 0) == (st["spmv_tiles"] > 0), (nr, d.value, a.value)


# ---- solves -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", x_cases.NAMES)
def test_solves_meet_the_stop_test_on_the_reference(name, hip):
    """Cold and warm, at block width 1 and in the default block loop with the degree and form the library picks: ||S (X_ref m / G0 - b)||_2 <=
    10 cg_tol at cg_tol = 1e-10 (the factor is the project's own).  I_macro and the dissipated power within power_ref.py's bounds evaluated on X_ref;
    the power bound gains 8 R sum|terms|, since the values the kernel multiplies are within 8 R of X_ref's."""
    import copy
    host, L = hip
    c = _case(name)
    p = copy.deepcopy(c["p"]); Vd = c["Vd"]
    assert p.cg_tol == 1e-10
    rp, ci, data = c["X64"]
    ref = c["ref"]
    for block in (1, 16):
        L.dkmc_set_x_block(block)
        p.solve_heating_global = False
        dev, gb = _device(c, hip)
        for start in ("cold", "warm"):
            dev.updatePower(gb, p, Vd)
            st = host.get_stats()
            m = get(gb, "atom_virtual_potentials").copy()
            assert np.all(np.isfinite(m))
            res = _scaled_residual(rp, ci, data, m, p.G0, p.X_loop_G, Vd)
            print("x-pin solve %s block %d %s: xb_width %d xb_fallback %d degree %d sweeps %d" % (name, block, start, st["xb_width"], st["xb_fallback"], st["xb_poly_used"], st["cg_iters_X"]))
            _note("stop test b%d %s" % (block, start), name, res, 10 * p.cg_tol)
            assert res <= 10 * p.cg_tol, (block, start)
            val, bound, terms = pr.imacro_reference(c["X64"], m)
            iw = _ratio(abs(dev.imacro - val), bound)
            _note("I_macro b%d %s" % (block, start), name, iw)
            assert iw <= 1 and len(terms) == p.num_atoms_first_layer
        p.solve_heating_global = True
        dev.updatePower(gb, p, Vd)
        m = get(gb, "atom_virtual_potentials").copy(); pw = get(gb, "site_power")
        e = pr.heating_entries(c["X64"], m, Vd)
        want, written, bound = pr.site_power_reference(c["X64"], m, Vd, ref["atom_site"], ref["metal"], len(pw), entries=e)
        _, mag, _ = pr.row_sums(e)
        vb = np.zeros(len(pw)); rows = np.arange(2, e["n"]); rows = rows[~ref["metal"][rows - 2]]
        vb[ref["atom_site"][rows - 2]] = 8 * max(R.values()) * mag[rows]
        pwst = _ratio(np.abs(pw - want)[written], (bound + vb)[written])
        _note("site power b%d" % block, name, pwst)
        assert pwst <= 1 and np.all(pw[~written] == 0.0), block


# ---- degenerate sets ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n320_v0", "n320_v1", "n319_v0"])
def test_degenerate_sets_have_no_tile(name, hip):
    """ns of 0 and 1 (a lone vacancy; a lone metal): no tile, xt_ns as in the table, and X is its neighbour part alone -- in both storage forms the
    exported matrix is the reference's, which has no tunnelling entry, and the solve meets the stop test on it."""
    host, L = hip
    c = _case(name)
    assert not np.isin(c["ref"]["kind"], (1, 2)).any()
    for fmt in (0, 1):
        L.dkmc_set_x_format(fmt)
        dev, gb = _device(c, hip)
        dev.updatePower(gb, c["p"], c["Vd"])
        st = host.get_stats()
        if fmt:
            assert st["xt_ns"] == c["counts"][1] and st["spmv_tiles"] == 0 and st["xt_subblocks"] == 0
            tiles, tval = _tiles(L)
            assert len(tiles) == 0 and len(tval) == 0
        X = host.get_last_X()
        assert np.array_equal(X[2].astype(LD)[c["ref"]["kind"] != 4], c["ref"]["val"][c["ref"]["kind"] != 4])
        m = get(gb, "atom_virtual_potentials")
        assert _scaled_residual(*c["X64"], m, c["p"].G0, c["p"].X_loop_G, c["Vd"]) <= 10 * c["p"].cg_tol
        val, bound, _ = pr.imacro_reference(c["X64"], m)
        assert abs(dev.imacro - val) <= bound


# ---- kept strips and the coefficient cache across a change of the vacancies ---------------------------------------------------------------------------
def _redrawn(c, extra, seed):
    """the case's structure with its vacancies drawn again, `extra` more of them; returns the case dict of the new state"""
    from devicekmc_amd import params as pm
    from devicekmc_amd.structure import Structure
    s = c["s"]
    el = s.element.copy()
    nV = int((el == pm.VACANCY).sum())
    el[el == pm.VACANCY] = pm.O_EL
    el[np.random.default_rng(seed).choice(np.flatnonzero(el == pm.O_EL), nV + extra, replace=False)] = pm.VACANCY
    c2 = _reference(Structure(el, s.x, s.y, s.z, dict(s.meta)), c["p"], c["cb"])
    c2.update(name=c["name"] + "+%d" % extra, Vd=c["Vd"], counts=(c2["ref"]["nM"], c2["ref"]["ns"]))
    return c2


@pytest.mark.parametrize("name", ["n191_v0", "n64_v0", "n64_l1_v1"])
def test_kept_strips_across_a_change_of_the_vacancies(name, hip):
    """nM = 257, 511, 638 with dkmc_set_x_static_tiles(1) and the self-check on: a solve, the vacancies drawn again with three more (ns 514 and 642
    cross a window and a row block), a second solve.  The all-metal strips are kept, the verify counters are 0, and the second assembly -- CSR, tile
    list and stored values -- equals a fresh device's bit for bit and the reference of the new state."""
    host, L = hip
    c = _case(name)
    c2 = _redrawn(c, 3, 5)
    assert c2["counts"] == (c["counts"][0], c["counts"][1] + 3)
    L.dkmc_set_x_static_tiles(1); L.dkmc_debug_x_static_verify(1)
    dev, gb = _device(c, hip)
    dev.updatePower(gb, c["p"], c["Vd"])
    info, ver = _static_info(L)
    assert info[0] == 1 and info[1] == c["counts"][0] // 256 > 0 and info[2] == 0 and info[6] in (FIRST, METALS) and info[7] == 0 and ver == [0, 0, 0, 0], (info, ver)
    put(gb, "site_element", c2["s"].element)
    dev.updateCharge(gb)
    assert np.array_equal(get(gb, "site_charge"), c2["charge"])
    dev.updatePower(gb, c["p"], c["Vd"])
    info, ver = _static_info(L)
    print("x-pin kept strips %s: info %s verify %s" % (name, info, ver))
    assert info[1] == c["counts"][0] // 256 and info[2] > 0 and info[4] > 0 and info[6] == KEPT, info
    assert info[7] == 0 and ver == [0, 0, 0, 0], (info, ver)
    assert host.get_stats()["xt_ns"] == c2["counts"][1]
    kept = (host.get_last_X(), _tiles(L))
    _check_csr(c2, kept[0], c2["name"] + "/kept")
    _check_store(c2, 1, L, c2["name"] + "/kept")
    dev2, gb2 = _device(c2, hip)
    dev2.updatePower(gb2, c2["p"], c2["Vd"])
    info, _ = _static_info(L)
    assert info[2] == 0 and info[6] != KEPT
    fresh = (host.get_last_X(), _tiles(L))
    for a, b in zip(kept[0] + kept[1], fresh[0] + fresh[1]):
        assert np.array_equal(a, b)


def test_coefficient_cache_across_a_change_of_the_vacancies(hip):
    """(64, 2, 257): a solve fills the cache of contact->trap integrals; then twelve vacancies go back to oxygen and fifteen oxygens become vacancies.
    The second assembly -- cached rows of the vacancies that stayed, new rows of the new ones -- meets the reference of the new state, and with
    dkmc_set_tcache_budget(0), every integral evaluated directly, the bits are the same."""
    from devicekmc_amd import params as pm
    from devicekmc_amd.structure import Structure
    host, L = hip
    c = _case("n64_v257")
    s = c["s"]
    el = s.element.copy()
    rng = np.random.default_rng(9)
    el[rng.choice(np.flatnonzero(el == pm.VACANCY), 12, replace=False)] = pm.O_EL
    el[rng.choice(np.flatnonzero(s.element == pm.O_EL), 15, replace=False)] = pm.VACANCY
    c2 = _reference(Structure(el, s.x, s.y, s.z, dict(s.meta)), c["p"], c["cb"])
    c2.update(name="n64_v257 redrawn", Vd=c["Vd"])
    assert c2["ref"]["ns"] == 771
    out = {}
    for budget in (-1, 0):
        L.dkmc_set_tcache_budget(budget)
        dev, gb = _device(c, hip)
        dev.updatePower(gb, c["p"], c["Vd"])
        first = host.get_last_X()
        cached = host.get_stats()["tcache_bytes"]
        put(gb, "site_element", el)
        dev.updateCharge(gb)
        assert np.array_equal(get(gb, "site_charge"), c2["charge"])
        dev.updatePower(gb, c["p"], c["Vd"])
        out[budget] = (first, host.get_last_X(), _tiles(L), cached)
        _check_csr(c, first, "n64_v257/budget%d" % budget)
        _check_csr(c2, out[budget][1], "redrawn/budget%d" % budget)
        _check_store(c2, 0, L, "redrawn/budget%d" % budget)
    assert out[-1][3] > 0
    for a, b in zip(out[-1][0] + out[-1][1] + out[-1][2], out[0][0] + out[0][1] + out[0][2]):
        assert np.array_equal(a, b)


# ---- the live view ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", [0, 1])
def test_every_tile_dead(poison, hip):
    """(64, 2, 0), metals only: every scaled entry is below 1e-4 (tests/test_x_ref.py), so under dkmc_set_x_tile_drop(1e-4) the live view holds no tile
    at all.  The view needs the fp32 image, which the assembly makes from tolerance 1e-8 on: the solves run at 1e-8 and meet 10 x that on X_ref, cold
    and warm, without a NaN -- also with every cell of the partial-sum array poisoned (a list fold that read a dead cell would carry the NaN on)."""
    import copy
    host, L = hip
    c = _case("n64_v0")
    p = copy.deepcopy(c["p"]); p.cg_tol = 1e-8
    L.dkmc_set_x_tile_drop(1e-4); L.dkmc_debug_poison_fold_cells(poison)
    dev, gb = _device(c, hip)
    for start in ("cold", "warm"):
        dev.updatePower(gb, p, c["Vd"])
        info = _live_info(L); st = host.get_stats()
        print("x-pin all dead %s poison %d: live info %s sweeps %d f64 rounds %d" % (start, poison, info, st["cg_iters_X"], st["x_tile_f64_rounds"]))
        assert info[0] == 1 and info[1] > 0 and info[2] == 0 and info[4] == 0 and info[5] == 0, info
        m = get(gb, "atom_virtual_potentials")
        assert np.all(np.isfinite(m)) and np.isfinite(dev.imacro)
        res = _scaled_residual(*c["X64"], m, p.G0, p.X_loop_G, c["Vd"])
        _note("stop test all dead %s" % start, "n64_v0/p%d" % poison, res, 10 * p.cg_tol)
        assert res <= 10 * p.cg_tol


def test_live_flags_and_masks_against_the_reference(hip):
    """(64, 2, 257) at theta = 1e-10, 1e-6 and 1e-4: a stored sub-block is live on its own when one of its entries reaches theta after scaling, (sS_i |t_ij|) sS_j,
    with the solve's own scaling (sS_out) and the reference's T; a tile is live when one of its sub-blocks is.  Sub-blocks whose largest scaled entry
    lies within 1e-12 relative of theta pass either way; they may be at most 1 % of the stored ones.  Then the solves under unit 0 and unit 1 report
    the reference's counts."""
    import copy
    from devicekmc_amd.lib import check
    host, L = hip
    theta = 1e-10
    c = _case("n64_v257")
    p = copy.deepcopy(c["p"]); p.cg_tol = 1e-8
    dev, gb = _device(c, hip)
    dev.updatePower(gb, p, c["Vd"])
    o = c[0]; ns = c["counts"][1]
    tiles, tval = _tiles(L)
    sS = np.zeros(ns)
    check(L.dkmc_xt_get_live(theta, None, sS.ctypes.data))
    d = c["ref"]["val"][c["ref"]["diag_pos"]][o["S"] + 2].astype(np.float64)
    assert np.all(np.abs(sS * np.sqrt(d) - 1) <= 1e-12)                     # the scaling is diag^-1/2
    A = np.where(o["up"], np.abs(o["T"]).astype(np.float64), 0.0)
    sc = (sS[:, None] * A) * sS[None, :]
    nsub_t = np.array([bin(int(v)).count("1") for v in tiles[:, 2]])
    stored = int(nsub_t.sum())
    for theta in THETAS:
        flags = np.zeros(len(tiles), dtype=np.int32); lmask = np.zeros(len(tiles), dtype=np.int32)
        check(L.dkmc_xt_get_live(theta, flags.ctypes.data, None))
        check(L.dkmc_xt_get_live_masks(theta, lmask.ctypes.data))
        want = np.zeros(len(tiles), dtype=np.int64); near = np.zeros(len(tiles), dtype=np.int64)
        for t, (k, w, mask, so) in enumerate(tiles):
            for q in range(8):
                if (mask >> q) & 1:
                    big = sc[32 * k:32 * k + 32, 256 * w + 32 * q:256 * w + 32 * q + 32].max()
                    if abs(big - theta) <= 1e-12 * theta:
                        near[t] |= 1 << q
                    elif big >= theta:
                        want[t] |= 1 << q
        excused = sum(bin(int(v)).count("1") for v in near)
        own = sum(bin(int(v)).count("1") for v in want)
        print("x-pin live masks n64_v257 theta %g: %d stored sub-blocks in %d tiles, %d live on their own in %d tiles, %d inside the guard band"
              % (theta, stored, len(tiles), own, (want != 0).sum(), excused))
        assert excused <= 0.01 * stored
        assert np.array_equal(lmask & ~near, want & ~near) and np.all((lmask & ~tiles[:, 2]) == 0)
        clear = near == 0
        assert np.array_equal((flags != 0)[clear], (want != 0)[clear]) and np.array_equal(flags != 0, lmask != 0)
        if theta == 1e-6:
            assert 0 < (want != 0).sum() < len(tiles) and own < nsub_t[want != 0].sum()      # live and dead tiles, dead sub-blocks inside live tiles
        if excused:
            continue
        L.dkmc_set_x_tile_drop(theta)
        for unit in (0, 1):
            L.dkmc_set_x_tile_drop_unit(unit)
            dev.updatePower(gb, p, c["Vd"])
            info = _live_info(L)
            streamed = own if unit else int(nsub_t[want != 0].sum())
            assert info[0] == (1 if (stored - streamed) * 64 >= stored else -2), (theta, unit, info)
            assert info[1] == len(tiles) and info[2] == (want != 0).sum() and info[3] == stored, (theta, unit, info)
            assert info[4] == nsub_t[want != 0].sum() and info[5] == own, (theta, unit, info)
            m = get(gb, "atom_virtual_potentials")
            assert _scaled_residual(*c["X64"], m, p.G0, p.X_loop_G, c["Vd"]) <= 10 * p.cg_tol, (theta, unit)
        L.dkmc_set_x_tile_drop(0.0); L.dkmc_set_x_tile_drop_unit(0)
