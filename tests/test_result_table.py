"""The host-side result table of the filament analyses and the copy-out body of their dkmc_copy_* entry points (csrc/result_table.h), on the CPU:
tests/cpu/result_table_check.cpp includes that header alone, is compiled with -fsanitize=address,undefined and run as a plain program; its output
is compared with rows written out here.  The rule, restated: rows = min(rows held, capacity), not below 0; *rows_out = rows unless rows_out is
NULL; every column that is not NULL gets its first `rows` elements, a NULL column is skipped, and 0 rows touch nothing.  The program allocates
every output buffer at exactly `rows` elements, so a body that writes one element more ends in an AddressSanitizer report.

The table of the check: int column c holds 100 * c + row, double column c holds c + row / 8 + 0.5; after "shrink" the rows left hold 1000 more.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NONE = "-"
# (rows held, capacity, mask of NULL arguments, what happens before the copy-out): (rows reported, the three int columns, the two double columns)
ROWS = {
    # capacity below, equal to and above the rows held
    (3, 2, 0, ()): (2, [[0, 1], [100, 101], [200, 201]], [[0.5, 0.625], [1.5, 1.625]]),
    (3, 3, 0, ()): (3, [[0, 1, 2], [100, 101, 102], [200, 201, 202]], [[0.5, 0.625, 0.75], [1.5, 1.625, 1.75]]),
    (3, 9, 0, ()): (3, [[0, 1, 2], [100, 101, 102], [200, 201, 202]], [[0.5, 0.625, 0.75], [1.5, 1.625, 1.75]]),
    (1, 1, 0, ()): (1, [[0], [100], [200]], [[0.5], [1.5]]),
    # capacity 0 and negative: 0 rows, nothing written (the buffers have no element)
    (3, 0, 0, ()): (0, [[], [], []], [[], []]),
    (3, -1, 0, ()): (0, [[], [], []], [[], []]),
    (3, -2147483648, 0, ()): (0, [[], [], []], [[], []]),
    # a table of 0 rows
    (0, 5, 0, ()): (0, [[], [], []], [[], []]),
    (0, 0, 0, ()): (0, [[], [], []], [[], []]),
    # NULL for some columns: the neighbours still right.  Bits 0 - 2 the int columns, 3 - 4 the double ones
    (3, 2, 0b00010, ()): (2, [[0, 1], NONE, [200, 201]], [[0.5, 0.625], [1.5, 1.625]]),
    (3, 3, 0b01101, ()): (3, [NONE, [100, 101, 102], NONE], [NONE, [1.5, 1.625, 1.75]]),
    (3, 3, 0b10000, ()): (3, [[0, 1, 2], [100, 101, 102], [200, 201, 202]], [[0.5, 0.625, 0.75], NONE]),
    (3, 3, 0b11111, ()): (3, [NONE, NONE, NONE], [NONE, NONE]),
    # NULL rows_out (bit 5): the columns all the same
    (3, 2, 0b100000, ()): (None, [[0, 1], [100, 101], [200, 201]], [[0.5, 0.625], [1.5, 1.625]]),
    (3, 0, 0b100000, ()): (None, [[], [], []], [[], []]),
    (3, 9, 0b100100, ()): (None, [[0, 1, 2], [100, 101, 102], NONE], [[0.5, 0.625, 0.75], [1.5, 1.625, 1.75]]),
    # resize to fewer rows after more: the new count, the new values, no row of the old ones
    (5, 9, 0, ("shrink", 2)): (2, [[1000, 1001], [1100, 1101], [1200, 1201]], [[1000.5, 1000.625], [1001.5, 1001.625]]),
    (5, 5, 0, ("shrink", 0)): (0, [[], [], []], [[], []]),
    (5, 1, 0, ("shrink", 2)): (1, [[1000], [1100], [1200]], [[1000.5], [1001.5]]),
    # and to more rows after fewer
    (2, 9, 0, ("shrink", 4)): (4, [[1000, 1001, 1002, 1003], [1100, 1101, 1102, 1103], [1200, 1201, 1202, 1203]],
                               [[1000.5, 1000.625, 1000.75, 1000.875], [1001.5, 1001.625, 1001.75, 1001.875]]),
    # clear, then copy-out
    (4, 9, 0, ("clear",)): (0, [[], [], []], [[], []]),
    (4, 9, 0b100000, ("clear",)): (None, [[], [], []], [[], []]),
}


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("result_table") / "result_table_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "devicekmc_amd", "csrc"), os.path.join(ROOT, "tests", "cpu", "result_table_check.cpp"), "-o", exe], check=True)

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (args, r.stdout, r.stderr)
        assert r.stderr == "", r.stderr                      # a sanitizer report goes here
        return dict(line.split(None, 1) if " " in line else (line, "") for line in r.stdout.splitlines())
    return run


def _column(text, kind):
    return NONE if text == NONE else [kind(v) for v in text.split()]


@pytest.mark.parametrize("case", sorted(ROWS), ids=lambda c: "-".join(str(v) for v in c[:3] + c[3]))
def test_copy_out_rows(check, case):
    held, capacity, mask, then = case
    rows, ints, doubles = ROWS[case]
    out = check("copy", held, capacity, mask, *then)
    assert out["rows"] == ("none" if rows is None else str(rows))
    assert [_column(out["i%d" % c], int) for c in range(3)] == ints
    assert [_column(out["d%d" % c], float) for c in range(2)] == doubles


@pytest.mark.parametrize("held,capacity,rows", [(3, 2, 2), (3, 3, 3), (3, 4, 3), (3, 0, 0), (0, 3, 0)])
def test_int_only_table(check, held, capacity, rows):
    out = check("ints", held, capacity)
    assert int(out["rows"]) == rows
    assert _column(out["i0"], int) == list(range(rows)) and _column(out["i1"], int) == [100 + r for r in range(rows)]
