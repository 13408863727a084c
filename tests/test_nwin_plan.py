"""The window plan of the LDS-windowed packed N product (csrc/nwin_plan.h), on the CPU: tests/cpu/nwin_plan_check.cpp includes that header alone, is
compiled with -fsanitize=address,undefined and run as a plain program.  For a synthetic pattern it forms every slot as k_xtb_npack does and asserts
that a slot either names the LDS row that holds exactly its column or is flagged and carries its global column; that a block's window (one segment)
lies in [0, m), never exceeds the cap and moves forward with the blocks; that the blocks cover every row once; and that with the cap at zero every
slot is flagged.  The counts it prints are compared with what the patterns imply."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 76 * 1024


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("nwin_plan") / "nwin_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "devicekmc_amd", "csrc"), os.path.join(ROOT, "tests", "cpu", "nwin_plan_check.cpp"), "-o", exe], check=True)

    def run(pattern, m, B, cap):
        r = subprocess.run([exe, pattern, str(m), str(B), str(cap)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stderr == "", (pattern, m, B, cap, r.stdout, r.stderr)      # a sanitizer report goes to stderr
        f = r.stdout.split()
        assert f[0] == "ok", r.stdout
        return {f[i]: int(f[i + 1]) for i in range(1, len(f), 2)}
    return run


# m = 3 (the driver rows plus one), m off multiples of 4, of 16 and of B, one block, several blocks, a last block of one row
SIZES = [3, 4, 5, 17, 63, 191, 192, 193, 577, 1000, 2001]


@pytest.mark.parametrize("pattern", ["band", "far10", "allfar", "wide", "random"])
@pytest.mark.parametrize("B", [128, 192, 256])
def test_every_slot_is_served_or_flagged(check, pattern, B):
    for m in SIZES:
        for cap in (CAP, 40 * 128, 16 * 128, 100, 0):
            out = check(pattern, m, B, cap)
            assert out["slots"] == out["inwin"] + out["flagged"] and out["blocks"] == -(-m // B), (m, cap, out)
            if cap < 128:
                assert out["inwin"] == 0 and out["winrows"] == 0, (m, cap, out)


def test_bands_fit_the_default_window(check):
    """Bands at +-85 and +-170 (+-1): a halo of (608 - 192) / 2 = 208 rows holds them all -- nothing is flagged; with B = 256 the halo is 176 rows and
    holds them too; the default plan (B = 320, halo 144) flags the outer band of the rows near a block's ends; a cap of one block (halo 0) leaves
    the +-85 band of the rows in the middle of a block in the window only."""
    for B in (192, 256):
        out = check("band", 2001, B, CAP)
        assert out["flagged"] == 0 and out["inwin"] == out["slots"] > 0, out
    out = check("band", 2001, 0, CAP)                                         # 0: no valid block size, the default
    assert out["blocks"] == -(-2001 // 320) and 0 < out["flagged"] < out["slots"] // 8, out
    out = check("band", 2001, 192, 192 * 128)
    assert 0 < out["flagged"] < out["slots"], out


def test_far_columns_are_flagged(check):
    """Columns at least 5000 rows away lie outside any window of 608 rows: only the zero-weight slots (the row itself) are served from LDS."""
    out = check("allfar", 20000, 192, CAP)
    assert out["flagged"] > 0 and out["inwin"] < out["slots"] // 4, out
    out10 = check("far10", 20000, 192, CAP)
    assert 0.05 < out10["flagged"] / out10["slots"] < 0.15, out10


def test_window_rows_of_a_plan(check):
    """Interior blocks copy 608 rows (192 + 2 x 208); the first and the last block lose the halo the panel does not have, their neighbours 16 rows of it."""
    out = check("band", 192 * 20, 192, CAP)
    assert out["blocks"] == 20 and out["winrows"] == 16 * 608 + 2 * (608 - 16) + 2 * (192 + 208), out
