"""bench.py as the driver runs it: a child process, one JSON line on stdout (the contract of the task description)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_line_single_gpu():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0",
                          "--no-cpu-baseline", "--no-aux"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 1 and line["rccl_world_size"] == 1 and line["steps"] == 1 and line["warmup"] == 0
    assert line["unit"] == "GF/s" and line["dtype"] == "f64" and line["value"] > 0 and line["ms_per_step"] > 0
    assert "chi_max=256" in line["config"]["workload"] and line["config"]["n_sites"] == 30
    roof = line["roofline"]
    assert roof["bound"] in ("hbm", "mfma") and 0 < roof["frac"] < 1 and roof["achieved"] > 0
    assert "mfma" in roof, "the MFMA kernels of the sweep are part of the line (BASELINE.json metric: ... + MFMA %)"


def test_bench_refuses_a_world_that_is_not_gpus():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0"],
                         capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode != 0 and "WORLD_SIZE=2" in (out.stderr + out.stdout)


def test_bench_site_shard_mode_single_gpu():
    """`--mode site-shard` (BASELINE.json configs[3]: d = 40, chi = 512) at N = 1: runs to its JSON line — round 4 found this mode
    faulting in 25 - 75 % of its runs (replay of the captured fill graph on a handle with asynchronous core export) — and the line
    says what is replicated, what shards and the bound that follows."""
    for _ in range(2):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--mode", "site-shard", "--gpus", "1", "--steps", "1",
                              "--warmup", "1"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, out.stdout[-2000:]
        line = json.loads(lines[0])
        assert line["n_gpus"] == 1 and line["config"]["chi_max"] == 512 and line["config"]["n_sites"] == 40
        am = line["amdahl"]
        assert am["replicated_ms"] > 0 and am["sharded_ms"] > 0 and am["speedup_bound_vs_n1"] >= 1.0
        assert line["scaling"] == "strong"


def _one_line(argv, timeout=900):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_patch_farm_mode_single_gpu():
    """`--mode patch-farm` (BASELINE.json configs[4] as stated: 64 statically projected patches, chi = 128, PaddedPatchFarm +
    DevicePatchExporter(group = 8), one all_gather_into_tensor) at N = 1: one JSON line with the per-rank times, the gathered bytes
    and the exposed gather time; every patch reaches chi.  No scaling claim at N = 1."""
    line = _one_line(["--mode", "patch-farm", "--gpus", "1", "--steps", "1", "--warmup", "1"])
    assert line["n_gpus"] == 1 and line["scaling"] == "strong" and line["unit"] == "patches/s"
    assert line["config"]["n_patches"] == 64 and line["config"]["chi_max"] == 128 and line["config"]["group"] == 8
    assert line["all_patches_reach_chi"] is True
    assert len(line["per_rank_ms_per_step"]) == 1 and line["per_rank_ms_per_step"][0] > 0
    assert line["gather_bytes_per_step"] >= 64 * 30 * 128 * 2 * 128 * 8
    assert 0 <= line["exposed_gather_ms_per_step"][0] < line["ms_per_step"]
    assert abs(line["value"] - 64 / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]


def test_bench_pi_shard_mode_single_gpu():
    """`--mode pi-shard` (candidate matrices of a host callback by column blocks, rrLU replicated) at N = 1: the
    unsharded callback path with its three costs side by side — the user function, the (absent) gather, the rrLU kernels."""
    line = _one_line(["--mode", "pi-shard", "--gpus", "1", "--steps", "1", "--warmup", "1"])
    assert line["n_gpus"] == 1 and line["scaling"] == "strong" and line["config"]["chi_max"] == 256
    assert line["callback_ms_per_step"][0] > 0 and line["rrlu_ms_per_step"][0] > 0 and line["gather_ms_per_step"][0] == 0.0
    assert line["callback_points_per_step_all_ranks"] > 1e7
    # (callback_ms is an ESTIMATE: points x the per-point cost calibrated on a probe batch; it is most of the step, and noise of the probe
    # may push it a few per cent past the measured wall time)
    assert 0.5 * line["ms_per_step"] < line["callback_ms_per_step"][0] < 1.25 * line["ms_per_step"]


def test_bench_dump_outputs(tmp_path):
    """--dump-outputs DIR: the tensor train, index sets and errors of the last timed sweep as float64 .npy files (64 MB at most), and
    --steps is the number of timed sweeps."""
    import numpy as np
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "0",
                          "--no-cpu-baseline", "--no-aux", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 2
    arrays = {f[:-4]: np.load(os.path.join(str(tmp_path), f)) for f in os.listdir(str(tmp_path)) if f.endswith(".npy")}
    assert all(a.dtype == np.float64 and a.size > 0 for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    n = line["config"]["n_sites"]
    assert len(arrays) == 5 + n + 2 * (n - 1) and "i_set_00" not in arrays and f"j_set_{n - 1:02d}" not in arrays
    links = [1] + [int(x) for x in arrays["link_dims"]] + [1]
    assert len(links) == n + 1 and max(links) == 256
    for p in range(n):
        assert arrays[f"site_tensor_{p:02d}"].shape == (links[p], 2, links[p + 1])
        assert p == 0 or arrays[f"i_set_{p:02d}"].shape == (links[p], p)
        assert p == n - 1 or arrays[f"j_set_{p:02d}"].shape == (links[p + 1], n - 1 - p)
        assert np.isfinite(arrays[f"site_tensor_{p:02d}"]).all()
    assert arrays["history_ranks"].tolist() == [256.0, 256.0] and np.isfinite(arrays["history_errors"]).all()


def test_bench_plain_run_does_only_the_headline_work():
    """A plain run times its steps and prints the line; what takes runs of its own after the timed steps (CPU baseline, aux block,
    exchange floor re-measured by tools/xcd_bench, HIP-event launch times) comes with --full only."""
    line = _one_line(["--gpus", "1", "--steps", "1", "--warmup", "0"])
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert "cpu_baseline" not in line and "aux" not in line
    roof = line["roofline"]
    assert roof["avg_launch_ms"] > 0 and roof["avg_launch_ms_hip_events"] is None
    assert roof["latency_view"]["exchange_floor_source"].endswith("not re-measured: a run without --full")


def test_bench_full_run_keeps_the_extras():
    """--full: the CPU baseline with its pivot check against the device, the aux block with its identity checks and the HIP-event
    launch times (--no-components leaves out aux.components, about a minute)."""
    line = _one_line(["--gpus", "1", "--steps", "1", "--warmup", "0", "--full", "--no-components"])
    cb = line["cpu_baseline"]
    assert cb["value"] > 0 and cb["pivots_identical_to_device"] is True
    aux = line["aux"]
    assert not [k for k in aux if k.endswith("_error")] and "components" not in aux
    assert aux["cfg2_time_to_solution_ms"] > 0 and aux["cfg5_patch_max_link_dim"] == 128 and aux["cfg4_size_max_link_dim"] == 512
    assert aux["cfg5_side_by_side_results_identical"] is True and aux["cfg5_group_results_identical"] is True
    roof = line["roofline"]
    assert roof["avg_launch_ms_hip_events"] > 0 and roof["latency_view"]["exchange_floor_us"] > 0
