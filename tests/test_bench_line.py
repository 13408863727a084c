"""bench.py's result line and --dump-outputs writer, on CPU: the line a driver parses must stay a few kB although the full record (kept in
the --detail file) is far larger, and the dumped outputs stay under their cap with a sample that does not change from run to run."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_result_line_of_a_full_record_is_compact():
    # a full N = 1 record of the default run (23 kB as one line)
    with open(os.path.join(ROOT, "profiles", "r05_bench_driver_command.json")) as f:
        out = json.load(f)
    assert len(json.dumps(out)) > 20000
    line = json.dumps(bench.result_line(out, "bench_detail.json"))
    assert len(line) <= 4096, len(line)
    got = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "config", "split_ms", "per_step", "roofline", "cpu_baseline"):
        assert got[k] == bench.result_line(out)[k], k
    assert got["value"] == out["value"] and got["ms_per_step"] == out["ms_per_step"] and got["steps"] == out["steps"]
    assert got["roofline"]["achieved"] == out["roofline"]["achieved"] and got["cpu_baseline"]["value"] == out["cpu_baseline"]["value"]
    assert got["detail"] == "bench_detail.json"


def test_save_outputs_float64_under_the_cap_and_seeded(tmp_path):
    n = 50000
    rng = np.random.default_rng(1)
    sites = {"site_charge": rng.integers(-1, 2, n).astype(np.int32), "site_potential_charge": rng.standard_normal(n)}
    scalars = {"dt": 1e-9, "I_macro": 2e-6, "T_bg": 300.0}
    # under the cap: every site, as float64
    bench.save_outputs(str(tmp_path / "all"), sites, scalars)
    a = np.load(tmp_path / "all" / "site_charge.npy")
    assert a.dtype == np.float64 and np.array_equal(a, sites["site_charge"])
    assert not (tmp_path / "all" / "site_index.npy").exists()
    assert np.load(tmp_path / "all" / "dt.npy").tolist() == [1e-9]
    # over the cap: the same seeded sample in every array and in every run, within the cap
    cap = 200000
    for d in ("s1", "s2"):
        bench.save_outputs(str(tmp_path / d), sites, scalars, cap_bytes=cap)
        assert sum(f.stat().st_size for f in (tmp_path / d).iterdir()) <= cap
    idx = np.load(tmp_path / "s1" / "site_index.npy")
    assert 0 < len(idx) < n and np.array_equal(idx, np.load(tmp_path / "s2" / "site_index.npy"))
    for name, arr in sites.items():
        assert np.array_equal(np.load(tmp_path / "s1" / (name + ".npy")), arr[idx.astype(np.int64)])
