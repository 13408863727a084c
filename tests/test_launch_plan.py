"""The batch plan, its poll count and the sampling rule of the solvers' host loops (csrc/launch_plan.h), on the CPU: tests/cpu/launch_plan_check.cpp
includes that header alone, is compiled with -fsanitize=address,undefined and run as a plain program; its output is compared with rows written out
here.  The rows follow from the rules of the five host loops, restated:

  doubling from 8             batch = 8; after a batch: if batch < 64: batch *= 2                                (K-CG, split-matrix CG, CSR CG without a hint)
  hint - 8                    batch = hint - 8 if hint > 24 else 8; after a batch: 8 if hint > 24 else doubling   (CG on X, CSR and tiled)
  three quarters              batch = max(4, 3 * hint // 4) if hint > 12 else 4; after a batch: 8 if hint > 12 else doubling   (block-CG)
  a poll before every batch and one that sees the stop word; a batch is enqueued while fewer iterations are enqueued than the solve needs
  position b of a batch is sampled if b < 64 and b % 8 == 0 (slot b // 8); a sample counts if its iteration index is below the final count
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (policy, hint, iterations): (batches, polls, iteration indices of the counted samples)
ROWS = {
    ("doubling", 8, 100): ([8, 16, 32, 64], 5, [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88, 96]),      # 13 = ceil(100 / 8): every batch starts on a multiple of 8
    ("minus8", 666, 670): ([658, 8, 8], 4, [0, 8, 16, 24, 32, 40, 48, 56, 658, 666]),                     # a first batch longer than 64: its first 64 only
    ("three_quarters", 40, 33): ([30, 8], 3, [0, 8, 16, 24, 30]),
    ("three_quarters", 0, 20): ([4, 8, 16], 4, [0, 4, 12]),                                               # 20 is not below 20
    # the thresholds: 24 is no hint, 25 is one (first batch 17); 12 is no hint, 13 is one (first batch 9)
    ("minus8", 24, 30): ([8, 16, 32], 4, [0, 8, 16, 24]),
    ("minus8", 25, 30): ([17, 8, 8], 4, [0, 8, 16, 17, 25]),
    ("three_quarters", 12, 10): ([4, 8], 3, [0, 4]),
    ("three_quarters", 13, 10): ([9, 8], 3, [0, 8, 9]),
    # a solve that needs no iteration is one poll; one iteration is one batch
    ("doubling", 8, 0): ([], 1, []),
    ("doubling", 8, 1): ([8], 2, [0]),
    ("minus8", 666, 0): ([], 1, []),
    ("three_quarters", 0, 1): ([4], 2, [0]),
    ("three_quarters", 400, 310): ([300, 8, 8], 4, [0, 8, 16, 24, 32, 40, 48, 56, 300, 308]),
    # doubling stops at 64
    ("doubling", 8, 200): ([8, 16, 32, 64, 64, 64], 7, list(range(0, 200, 8))),
    ("doubling", 8, 120): ([8, 16, 32, 64], 5, list(range(0, 120, 8))),                                   # exactly the iterations of four batches: no fifth
}


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("launch_plan") / "launch_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "devicekmc_amd", "csrc"), os.path.join(ROOT, "tests", "cpu", "launch_plan_check.cpp"), "-o", exe], check=True)

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (args, r.stdout, r.stderr)
        assert r.stderr == "", r.stderr                      # a sanitizer report goes here
        return r.stdout
    return run


@pytest.mark.parametrize("case", sorted(ROWS), ids=lambda c: "%s-%d-%d" % c)
def test_plan_rows(check, case):
    batches, polls, samples = ROWS[case]
    out = dict(line.split(None, 1) if " " in line else (line, "") for line in check("plan", *case).splitlines())
    assert [int(v) for v in out["batches"].split()] == batches
    assert int(out["polls"]) == polls
    assert [int(v) for v in out["samples"].split()] == samples


def heat_csr_polls(iters):                                   # polls of a CSR solve without a hint (what heat.hip reports as its host synchronisations), stated on its own
    n, launched, batch = 1, 0, 8
    while launched < iters: launched += batch; n += 1; batch = batch * 2 if batch < 64 else batch
    return n


def test_polls_of_the_doubling_plan(check):
    got = [int(v) for v in check("polls", "doubling", 8, 0, 300).split()]
    assert got == [heat_csr_polls(i) for i in range(301)]
