"""The residence-time event loop as its sequential definition (oracle/kmc_oracle.c: okmc_execute_events), in plain numpy, for tables whose sums
are exact.  Test infrastructure: tests/test_event_loop_ref.py pins it to the oracle, tests/test_gpu_event_loop.py compares the device loop with it.

The table is an integer array in units of `scale` (a power of two), or an np.longdouble array (scale 1) for a table that came out of exp().  Per event
    Psum   = the sum of the table (exact for integers),
    number = u * Psum, ONE double multiplication,
    slot   = the first slot whose inclusive prefix exceeds number; the last positive slot if there is none; none at all if no rate is positive,
the event class follows from the two elements at execution time, every slot whose row or target is i or j is zeroed by a scan over the whole
table, and dt = -log(u2) / Psum.  The loop stops when !(dt < 1 / freq), when no positive rate is left, or when the draws run out
(2 * n_events + 1 >= n_uniform, checked before each selection)."""
from fractions import Fraction

import numpy as np

DEFECT, OXYGEN_DEFECT, VACANCY, O_EL = 0, 1, 2, 3
EV_GEN, EV_REC, EV_VDIFF, EV_IDIFF, EV_NULL = 0, 1, 2, 3, 4


def event_class(ei, ej):
    if ei == DEFECT and ej == O_EL:
        return EV_GEN
    if ei == OXYGEN_DEFECT and ej == VACANCY:
        return EV_REC
    if ei == VACANCY and ej == O_EL:
        return EV_VDIFF
    if ei == OXYGEN_DEFECT and ej == DEFECT:
        return EV_IDIFF
    return EV_NULL


def slot_classes(neigh, element):
    """The class of every slot from the elements as they are (EV_NULL for pads): the ev_type table the oracle wants beside the rates."""
    element = np.asarray(element)
    N = len(element)
    neigh = np.asarray(neigh).reshape(N, -1)
    ei = np.repeat(element[:, None], neigh.shape[1], axis=1)
    ej = element[np.clip(neigh, 0, N - 1)]
    t = np.full(neigh.shape, EV_NULL, dtype=np.int32)
    live = neigh >= 0
    for cls, a, b in ((EV_GEN, DEFECT, O_EL), (EV_REC, OXYGEN_DEFECT, VACANCY), (EV_VDIFF, VACANCY, O_EL), (EV_IDIFF, OXYGEN_DEFECT, DEFECT)):
        t[live & (ei == a) & (ej == b)] = cls
    return t.reshape(-1)


class EventLoop:
    """The state of one loop: table, elements, charges.  A caller that chooses its draws from the state (prefix(), psum) drives it with step()."""

    def __init__(self, table, neigh, element, charge, freq, scale=1.0):
        self.N = len(element)
        self.neigh = np.asarray(neigh, dtype=np.int64).reshape(-1)
        assert len(self.neigh) % self.N == 0
        self.nn = len(self.neigh) // self.N
        table = np.asarray(table).reshape(-1)
        assert len(table) == len(self.neigh)
        self.exact = table.dtype.kind in "iu" or table.dtype == object
        if self.exact:
            assert table.astype(np.float64).sum() < 2.0 ** 52             # every partial sum is then exact in every order
            self.P = table.astype(np.int64)
        else:
            self.P = table.astype(np.longdouble)
        assert (self.P >= 0).all()
        self.row = np.repeat(np.arange(self.N, dtype=np.int64), self.nn)
        self.element = np.asarray(element, dtype=np.int32).copy()
        self.charge = np.asarray(charge, dtype=np.int32).copy()
        self.freq = float(freq)
        self.scale = float(scale)
        self.log, self.margin, self.psums = [], [], []
        self._cum = None

    def prefix(self):
        """Inclusive prefix sums of the table as it is now (cached until the next event)."""
        if self._cum is None:
            self._cum = np.cumsum(self.P)
        return self._cum

    @property
    def psum(self):
        c = self.prefix()
        return int(c[-1]) if self.exact else c[-1]

    def select(self, u):
        """(slot, exact distance of `number` to the nearer edge of its bucket, in table units), or None when no rate is positive."""
        cum = self.prefix()
        Psum = cum[-1]
        if not Psum > 0:
            return None
        number = np.float64(u) * np.float64(Psum)                       # one double multiplication
        slot = int(np.searchsorted(cum, number, side="right"))          # integers below 2^52 are doubles: the comparison is exact
        if slot >= len(cum):
            slot = int(np.flatnonzero(self.P > 0)[-1])                  # no prefix exceeds number: the last positive slot
        below = cum[slot - 1] if slot else 0
        if self.exact:
            a, b = Fraction(float(number)) - int(below), int(cum[slot]) - Fraction(float(number))
            margin = float(min(a, b))                                   # a difference of a double and an integer below it: a double
            assert Fraction(margin) == min(a, b)
        else:
            margin = float(min(np.longdouble(number) - below, cum[slot] - np.longdouble(number)))
        return slot, margin

    def step(self, u, u2):
        """One event on draws (u, u2): returns dt, or None (and changes nothing) when no rate is positive."""
        sel = self.select(u)
        if sel is None:
            return None
        slot, margin = sel
        Psum = np.float64(self.prefix()[-1]) * np.float64(self.scale)
        i, j = slot // self.nn, int(self.neigh[slot])
        assert j >= 0, "a pad slot holds a positive rate"
        ei, ej, qi, qj = self.element[i], self.element[j], self.charge[i], self.charge[j]
        cls = event_class(ei, ej)
        if cls == EV_GEN:
            self.element[i], self.element[j], self.charge[i], self.charge[j] = OXYGEN_DEFECT, VACANCY, -2, 2
        elif cls == EV_REC:
            self.element[i], self.element[j], self.charge[i], self.charge[j] = DEFECT, O_EL, 0, 0
        elif cls in (EV_VDIFF, EV_IDIFF):
            self.element[i], self.element[j], self.charge[i], self.charge[j] = ej, ei, qj, qi
        self.log.append((slot, i, j, cls)); self.margin.append(margin); self.psums.append(float(Psum))
        dead = (self.row == i) | (self.row == j) | (self.neigh == i) | (self.neigh == j)      # the whole table, as zero_out_events scans it
        self.P[dead] = 0
        self._cum = None
        with np.errstate(divide="ignore"):
            return float(-np.log(np.float64(u2)) / Psum)


def run(table, neigh, element, charge, freq, draws, scale=1.0, loop=None):
    """The loop on an explicit list of draws (two per event).  loop: an EventLoop to go on with (the resume of the device); its log grows.
    Returns log [n, 4] (slot, i, j, type) of THIS call, n_events, dt of the last event (0.0 without one, inf when the table ran dry),
    exhausted, dry, the elements and charges afterwards, the margins of this call's events, and the loop."""
    lp = loop if loop is not None else EventLoop(table, neigh, element, charge, freq, scale)
    first = len(lp.log)
    n, dt, exhausted, dry = 0, 0.0, False, False
    inv_freq = 1 / np.float64(lp.freq)
    while True:
        if 2 * n + 1 >= len(draws):
            exhausted = True
            break
        d = lp.step(draws[2 * n], draws[2 * n + 1])
        if d is None:
            dry, dt = True, float("inf")
            break
        dt = d
        n += 1
        if not dt < inv_freq:
            break
    return dict(log=np.array(lp.log[first:], dtype=np.int32).reshape(-1, 4), n_events=n, dt=dt, exhausted=exhausted, dry=dry,
                element=lp.element.copy(), charge=lp.charge.copy(), margin=np.array(lp.margin[first:]), loop=lp)
