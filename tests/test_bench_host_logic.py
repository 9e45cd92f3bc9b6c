"""Host-side logic of bench.py that needs no GPU: the shape of the JSON lines it assembles around the measurements (the compact
form of an extra workload, the one-line error report of a failed multi-rank run, the host topology of `cpu_baseline`)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _args(**kw):
    base = dict(gpus=1, steps=10, warmup=3, workload="as", prior=False, quick=False, headline_only=False, dist_single=False,
                samples_total=512, kernel_point=False, eig_large=False, full=False, dump_outputs=None)
    base.update(kw)
    return argparse.Namespace(**base)


def test_extras_ride_on_the_default_run_only():
    """The extra workloads ride on the default config-4 command with --full; a plain run is the headline alone."""
    assert bench.kernel_extras_wanted(_args(full=True), 1)
    assert not bench.kernel_extras_wanted(_args(), 1)
    for kw in (dict(headline_only=True), dict(workload="pod"), dict(prior=True), dict(dist_single=True), dict(samples_total=64)):
        assert not bench.kernel_extras_wanted(_args(full=True, **kw), 1)
    assert not bench.kernel_extras_wanted(_args(full=True), 2)


def test_plain_run_options():
    """--full is off by default, --dump-outputs takes a directory, --steps sets the timed steps."""
    argv = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"]
        a = bench.parse_args()
        assert not a.full and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
        sys.argv = ["bench.py", "--full", "--dump-outputs", "out_dir"]
        a = bench.parse_args()
        assert a.full and a.dump_outputs == "out_dir"
    finally:
        sys.argv = argv


def test_dump_outputs_small_block_is_written_whole(tmp_path):
    rng = np.random.default_rng(0)
    d, U = rng.standard_normal(12), rng.standard_normal((500, 12))
    names = bench.dump_outputs(str(tmp_path / "o"), d, U)
    assert names == ["eigenvalues", "eigenvectors"]
    assert sorted(os.listdir(tmp_path / "o")) == ["eigenvalues.npy", "eigenvectors.npy"]
    for name, ref in (("eigenvalues", d), ("eigenvectors", U)):
        a = np.load(tmp_path / "o" / (name + ".npy"))
        assert a.dtype == np.float64
        np.testing.assert_array_equal(a, ref)


def test_dump_outputs_large_block_is_a_fixed_row_sample_within_budget(tmp_path, monkeypatch):
    """Beyond the budget the eigenvectors are a seeded sample of rows that depends on the shape only: two runs (two builds) write
    the same rows, and everything written stays under 64 MB at the flagship's shape."""
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 8 * 64 * 1000)                 # 1000 rows of 64
    rng = np.random.default_rng(1)
    U = rng.standard_normal((5000, 64))
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), np.arange(64.0), U)
    rows = np.load(tmp_path / "a" / "eigenvector_rows.npy")
    assert rows.dtype == np.float64 and rows.shape == (1000,) and np.all(np.diff(rows) > 0)
    np.testing.assert_array_equal(rows, np.load(tmp_path / "b" / "eigenvector_rows.npy"))
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "eigenvectors.npy"), U[rows.astype(np.int64)])
    monkeypatch.undo()
    N, r = 200000, 64                                                               # config 4
    rows_max = bench.DUMP_BUDGET_BYTES // (8 * r)
    assert rows_max < N and 8 * (rows_max * r + rows_max + r) < 64 * 2 ** 20


def test_compact_form_of_an_extra_workload():
    line = {"value": 4.1, "unit": "GDoF*rank/s", "ms_per_step": 15.5, "median_ms_per_step": 15.4, "steps": 5, "warmup": 2,
            "config": {"workload": "config3 PODProjector"}, "literal_T_ms_per_step": 20.0,
            "roofline": {"kernel": "k_tsgemm_tn m=2048 k=138 N=500000", "bound": "mfma", "achieved": 64.0, "peak": 78.6, "unit": "TFLOP/s",
                         "frac": 0.81, "avg_launch_ms": 4.4, "traffic": None, "extra": 1},
            "parity": {"eig_rel_err_vs_oracle": 4e-13, "note": "long text", "oracle_form": "x"},
            "phases_ms_per_step": {"apply_A": 9.0},
            "cpu_baseline": {"value": 0.01, "unit": "GDoF*rank/s", "kind": "port", "cores": 64, "threads": 256, "physical_cores": 128,
                             "sockets": 2, "best_setting": "threads_all", "seconds_full_estimate": 3.8, "sample": "s",
                             "reference_style": {"best_single_setting_value": 6e-4,
                                                 "composite_of_per_component_best_settings": {"value": 7e-4}}, "blas3": {}},
            "communicator": {"ranks": 1, "transport": "rccl"}}
    c = bench._compact(line)
    assert c["workload"] == "config3 PODProjector" and c["ms_per_step"] == 15.5 and c["roofline"]["frac"] == 0.81
    assert "extra" not in c["roofline"] and "note" not in c["parity"] and c["parity"]["eig_rel_err_vs_oracle"] == 4e-13
    assert c["cpu_baseline"]["reference_style_composite_of_per_component_best_settings_value"] == 7e-4
    assert c["cpu_baseline"]["reference_style_best_single_setting_value"] == 6e-4 and c["cpu_baseline"]["physical_cores"] == 128
    assert c["communicator"]["transport"] == "rccl"
    json.dumps(c)
    bare = bench._compact({"value": 1.0, "config": {"workload": "w"}})             # nothing optional present
    assert bare["roofline"]["frac"] is None and bare["parity"] == {} and "cpu_baseline" not in bare


def test_error_line_keeps_the_contract_keys():
    e = bench._error_line(_args(gpus=8), "rank 3 exited with code 7", rank_exit_codes=[0, 0, 0, 7])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "error"):
        assert key in e
    assert e["value"] is None and e["n_gpus"] == 8 and e["rank_exit_codes"][3] == 7
    json.dumps(e)


def test_cpu_topology_is_sane():
    t = bench._cpu_topology()
    assert t["threads"] >= 1 and 1 <= t["physical_cores"] <= max(t["threads"], t["physical_cores"]) and t["sockets"] >= 1
    assert t["physical_cores"] >= t["sockets"]


def test_cpu_quota_of_the_container_is_read_from_the_cgroup(tmp_path):
    """bench.py keeps the host BLAS pool inside what the cgroup lets the process run: cgroup v2 `cpu.max`
    ("quota period" or "max period"), cgroup v1 cfs files, nothing at all."""
    f = tmp_path / "cpu.max"
    f.write_text("1600000 100000\n")
    assert bench._cpu_quota(str(f), str(tmp_path / "none")) == 16
    f.write_text("max 100000\n")
    assert bench._cpu_quota(str(f), str(tmp_path / "none")) is None
    f.write_text("50000 100000\n")
    assert bench._cpu_quota(str(f), str(tmp_path / "none")) == 1                  # half a CPU still means one thread
    v1 = tmp_path / "v1"
    v1.mkdir()
    (v1 / "cpu.cfs_quota_us").write_text("800000\n")
    (v1 / "cpu.cfs_period_us").write_text("100000\n")
    assert bench._cpu_quota(str(tmp_path / "missing"), str(v1)) == 8
    (v1 / "cpu.cfs_quota_us").write_text("-1\n")
    assert bench._cpu_quota(str(tmp_path / "missing"), str(v1)) is None

