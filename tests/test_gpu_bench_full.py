"""What a plain `bench.py` run measures and what --full adds to it, on the 9 399-site device (seconds on the GPU).  A plain run times the
headline alone; every block beside it (other configurations, CPU baselines, PMC child runs, models) belongs to --full."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

# blocks of the N = 1 record that run or measure something beside the timed steps
FULL_BLOCKS = ("plain_block_loop", "x_poly_gain", "strong_scaling_model", "reference_start_vector", "warm_start_gain", "reference_order_cg",
               "block_cg_gain", "gpu_over_cpu", "device_7p5nm", "scale_points")


def run_bench(tmp_path, *extra):
    detail = str(tmp_path / "detail.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "2.5nm", "--steps", "2", "--warmup", "1",
                        "--detail", detail] + list(extra), capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    with open(detail) as f:
        return line, json.load(f)


def test_plain_run_measures_the_headline_alone(tmp_path):
    line, rec = run_bench(tmp_path, "--dump-outputs", str(tmp_path / "out"))
    assert line["metric"] == "KMC steps/sec" and line["value"] > 0 and line["ms_per_step"] > 0 and line["steps"] == 2
    assert line["higher_is_better"] is True and line["dtype"] == "f64" and line["unit"] == "KMC steps/s"
    assert rec["roofline"]["launches"] > 0 and rec["roofline"]["traffic"] is None
    assert rec["cpu_baseline"] is None
    assert [k for k in FULL_BLOCKS if k in rec] == []
    assert os.path.exists(tmp_path / "out" / "site_potential_charge.npy")


def test_full_adds_the_blocks_beside_the_headline(tmp_path):
    # the cheap blocks of --full at this size; the --no-* options still skip single blocks of a --full run
    _, rec = run_bench(tmp_path, "--full", "--no-device", "--no-pmc", "--no-reference-order", "--no-cpu-baseline")
    assert rec["plain_block_loop"]["steps"] > 0 and rec["reference_start_vector"]["steps"] > 0
    assert "device_7p5nm" not in rec and "reference_order_cg" not in rec and rec["cpu_baseline"] is None
