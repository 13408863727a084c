"""The size rule of dkmc_set_x_stop_form(2) (csrc/xtb_precond.h: xtb_stop_rule; host code, no GPU): the norm stop test runs from 96 000 rows on -- the
geometric midpoint of the two measured sizes it separates (57 782 rows: no gain, 160 526 rows: + 9.8 %; profiles/ab_bench_x_stop_form.txt)."""
import math

from devicekmc_amd import lib


def test_gate_and_measured_sizes():
    L = lib.load()
    assert [L.dkmc_xtb_stop_rule(m) for m in (0, 1, 2, 6422, 57782, 95999)] == [0] * 6
    assert [L.dkmc_xtb_stop_rule(m) for m in (96000, 160526, 642101, 2 ** 31 - 1)] == [1] * 4
    assert abs(math.sqrt(57782 * 160526) / 96000 - 1) < 0.01
