"""numpy restatement of the event table with the local-temperature rate models (dkmc_set_event_temperature) and of the rate census
(dkmc_event_rate_census), the reference the GPU tests compare against.  The CPU oracle has no temperature model; tests/test_event_temp_ref.py
pins mode 0 of this restatement to the oracle's build_event_list before it is trusted.

slot_tables follows kmc_events.cu:52-122 term by term -- the integer division in the recombination energy (:77), layer[j] for every class
(:98) --, with the reference authors' commented-out kinetic term (:65,81,99,118) as mode 1 and Arrhenius on the site temperature as mode 2.  The
deciding site is j for generation and i for recombination, vacancy diffusion and ion diffusion."""
import math

import numpy as np

KB = 8.617333262e-5
Q = 1.60217663e-19
DEFECT, OXYGEN_DEFECT, VACANCY, O_EL = 0, 1, 2, 3
EV_GEN, EV_REC, EV_VDIFF, EV_IDIFF, EV_NULL = 0, 1, 2, 3, 4

_erfc = np.frompyfunc(math.erfc, 1, 1)


def _round_half_away(f):
    return np.sign(f) * np.floor(np.abs(f) + 0.5)          # C round()


def _site_dist(xi, yi, zi, xj, yj, zj, lattice, pbc):
    if pbc:
        dx = xi - xj
        fy = (yi - yj) / lattice[1]; fy = fy - _round_half_away(fy)
        fz = (zi - zj) / lattice[2]; fz = fz - _round_half_away(fz)
        dy, dz = fy * lattice[1], fz * lattice[2]
        return np.sqrt(dx * dx + dy * dy + dz * dz)
    dx, dy, dz = xj - xi, yj - yi, zj - zi
    return np.sqrt(dx * dx + dy * dy + dz * dz)


def _v_solve(r, charge, sigma, k):
    e = _erfc(r / (sigma * math.sqrt(2.0))).astype(np.float64) if len(r) else np.zeros(0)
    return charge * e * k * Q / r


def slot_tables(mode, neigh, layer, lattice, pbc, T_bg, freq, sigma, k, x, y, z, pb, pc, element, charge, E_gen, E_rec, E_Vdiff, E_Odiff,
                temperature=None):
    """(types int32 [N * nn], P float64 [N * nn], n_bad).  mode 0: temperature unused.  Modes 1, 2: a class slot whose deciding temperature is
    not finite or not > 0 keeps its type, gets P = 0 and counts in n_bad."""
    neigh = np.asarray(neigh).reshape(len(element), -1)
    N, nn = neigh.shape
    types = np.full(N * nn, EV_NULL, dtype=np.int32)
    P = np.zeros(N * nn)
    flat = neigh.reshape(-1)
    slot = np.flatnonzero((flat >= 0) & (flat < N))
    i, j = slot // nn, flat[slot]
    ei, ej = element[i], element[j]
    cls = np.full(len(slot), EV_NULL)
    cls[(ei == DEFECT) & (ej == O_EL)] = EV_GEN
    cls[(ei == OXYGEN_DEFECT) & (ej == VACANCY)] = EV_REC
    cls[(ei == VACANCY) & (ej == O_EL)] = EV_VDIFF
    cls[(ei == OXYGEN_DEFECT) & (ej == DEFECT)] = EV_IDIFF
    keep = cls != EV_NULL
    slot, i, j, cls = slot[keep], i[keep], j[keep], cls[keep]
    dist = 1e-10 * _site_dist(x[i], y[i], z[i], x[j], y[j], z[j], lattice, pbc)
    dphi = (pb[i] + pc[i]) - (pb[j] + pc[j])
    qi, qj, lj = charge[i].astype(np.int64), charge[j].astype(np.int64), layer[j]
    En, E0 = np.zeros(len(slot)), np.zeros(len(slot))
    m = cls == EV_GEN
    En[m] = 2 * dphi[m]; E0[m] = np.asarray(E_gen)[lj[m]]
    m = cls == EV_REC
    cs = qi[m] - qj[m]
    half = np.sign(cs) * (np.abs(cs) // 2)                  # C integer division truncates towards zero (kmc_events.cu:77)
    En[m] = cs * (dphi[m] + half * _v_solve(dist[m], 2, sigma, k)); E0[m] = np.asarray(E_rec)[lj[m]]
    m = cls == EV_VDIFF
    self_ = np.where(qi[m] != 0, _v_solve(dist[m], qi[m].astype(np.float64), sigma, k), 0.0)
    En[m] = (qi[m] - qj[m]) * (dphi[m] + self_); E0[m] = np.asarray(E_Vdiff)[lj[m]]          # layer of j (kmc_events.cu:98)
    m = cls == EV_IDIFF
    self_ = np.where(qi[m] != 0, _v_solve(dist[m], 2, sigma, k), 0.0)
    En[m] = (qi[m] - qj[m]) * (dphi[m] - self_); E0[m] = np.asarray(E_Odiff)[lj[m]]
    n_bad = 0
    with np.errstate(over="ignore", invalid="ignore"):
        if mode == 0:
            EA = E0 - En - 0
            rate = np.exp(-1 * EA / (KB * T_bg)) * freq
        else:
            T_s = np.where(cls == EV_GEN, temperature[j], temperature[i])
            bad = ~(np.isfinite(T_s) & (T_s > 0))
            T_use = np.where(bad, 1.0, T_s)
            if mode == 1:
                Ekin = KB * (T_use - T_bg)
                EA = E0 - En - Ekin
                rate = np.exp(-1 * EA / (KB * T_bg)) * freq
            else:
                EA = E0 - En - 0
                rate = np.exp(-1 * EA / (KB * T_use)) * freq
            rate[bad] = 0.0
            n_bad = int(bad.sum())
    types[slot] = cls
    P[slot] = rate
    return types, P, n_bad


def deciding_temperature(neigh, element, temperature):
    """T_s per slot (NaN where the slot has no event class), and the class per slot."""
    neigh = np.asarray(neigh).reshape(len(element), -1)
    N, nn = neigh.shape
    flat = neigh.reshape(-1)
    ok = (flat >= 0) & (flat < N)
    j = np.where(ok, flat, 0)
    i = np.repeat(np.arange(N), nn)
    ei, ej = element[i], element[j]
    cls = np.full(N * nn, EV_NULL)
    cls[ok & (ei == DEFECT) & (ej == O_EL)] = EV_GEN
    cls[ok & (ei == OXYGEN_DEFECT) & (ej == VACANCY)] = EV_REC
    cls[ok & (ei == VACANCY) & (ej == O_EL)] = EV_VDIFF
    cls[ok & (ei == OXYGEN_DEFECT) & (ej == DEFECT)] = EV_IDIFF
    T_s = np.where(cls == EV_GEN, temperature[j], temperature[i])
    return np.where(cls == EV_NULL, np.nan, T_s), cls


def census(neigh, element, ev_prob, temperature=None):
    """The 16 doubles of dkmc_event_rate_census (include/devicekmc_hip.h), sums by math.fsum."""
    ev_prob = np.asarray(ev_prob, dtype=np.float64).reshape(-1)
    T = np.zeros(len(element)) if temperature is None else np.asarray(temperature, dtype=np.float64)
    T_s, cls = deciding_temperature(neigh, element, T)
    info = np.zeros(16)
    finite = np.isfinite(ev_prob)
    live = finite & (ev_prob > 0)
    for c in range(4):
        m = live & (cls == c)
        info[c] = m.sum()
        info[4 + c] = math.fsum(ev_prob[m])
        if temperature is not None:
            info[8 + c] = math.fsum(ev_prob[m] * T_s[m])
    if live.any():
        info[12] = ev_prob[live].max()
        info[13] = np.flatnonzero(live & (ev_prob == info[12]))[0]
    else:
        info[13] = -1
    info[14] = (~finite).sum()
    info[15] = info[:4].sum()
    return info


def ball_field(x, y, z, T_bg, dT=300.0, R=8.0):
    """T = T_bg + dT exp(-r^2 / R^2) inside a ball of radius R around the centre of the cell, exactly T_bg outside."""
    c = [(a.min() + a.max()) / 2 for a in (x, y, z)]
    r2 = (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2
    T = np.full(len(x), float(T_bg))
    inside = r2 < R * R
    T[inside] = T_bg + dT * np.exp(-r2[inside] / (R * R))
    return T


def randomised_state(seed, element, x):
    """The site states and rough potentials of test_gpu_parity.test_randomised_event_engine: 300 vacancies, 200 oxygen ions, |dphi| up to
    ~2 V between neighbours.  Returns (element, pot_boundary, pot_charge); the charges follow from update_charge."""
    rng = np.random.default_rng(seed)
    el = np.array(element, dtype=np.int32)
    ox = np.nonzero(el == O_EL)[0]; dd = np.nonzero(el == DEFECT)[0]
    el[rng.choice(ox, 300, replace=False)] = VACANCY
    el[rng.choice(dd, 200, replace=False)] = OXYGEN_DEFECT
    N = len(el)
    pb = np.linspace(-2.5, 2.5, N)[np.argsort(np.argsort(x))] + 0.3 * rng.standard_normal(N)
    pc = 0.2 * rng.standard_normal(N)
    return el, pb, pc


def oracle_tables(o, mode, temperature=None, T_bg=None):
    """slot_tables on the state of an OracleKMC."""
    p = o.p
    return slot_tables(mode, o.neigh, o.layer, o.lattice, int(p.pbc), o.T_bg if T_bg is None else T_bg, p.freq, p.sigma, p.k, o.x, o.y, o.z,
                       o.pot_boundary, o.pot_charge, o.element, o.charge, o.E_gen, o.E_rec, o.E_Vdiff, o.E_Odiff, temperature)
