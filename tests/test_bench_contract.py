"""bench.py's bookkeeping that can be checked without a GPU: the algorithmic work per scene is SURVEY.md 8(d)'s (493.4 GFLOP / 6.61 GB at
the metric configuration, 131.3 GFLOP / 1.86 GB at configs[1]), the workloads are the configurations BASELINE.json names, the committed
counter files carry the stamp of the library they were measured on, the committed default line has the contract's keys, and
--dump-outputs samples the same elements every time within its budget. On the GPU: a plain run times exactly --steps steps and
writes what its last step computed."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(REPO, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_algorithmic_work_is_surveys_formula():
    b = _bench()
    N, C, H, W, T = b.WORKLOADS["metric"]
    assert (N, C, H, W, T) == (4, 64, 200, 704, 20)                      # BASELINE.json metric
    fl, by = b.algorithmic_work(N, C, H * W, T)
    assert fl / 1e9 == pytest.approx(493.4, abs=0.1) and by / 1e9 == pytest.approx(6.61, abs=0.01)
    N, C, H, W, T = b.WORKLOADS["cfg2"]
    assert (N, C, H, W, T) == (2, 64, 200, 704, 10)                      # BASELINE.json configs[1]
    fl, by = b.algorithmic_work(N, C, H * W, T)
    assert fl / 1e9 == pytest.approx(131.3, abs=0.1) and by / 1e9 == pytest.approx(1.86, abs=0.01)
    assert b.HBM_PEAK_GBS == 8000.0 and b.FP32_PEAK_TFLOPS == pytest.approx(157.3)


def test_committed_counter_files_are_stamped_and_consistent():
    for name in ("r4_pmc_traffic.json", "r4_pmc_sq.json", "r4_pmc_insts.json"):
        d = json.load(open(os.path.join(REPO, "profiles", name)))
        assert d.get("workload") == "metric" and len(d.get("library_src", "")) == 16, name
    t = json.load(open(os.path.join(REPO, "profiles", "r4_pmc_traffic.json")))
    fam = t["conv8h_family"]
    # counter traffic per launch within a few percent of the algorithmic bytes of the family's launch mix (122.55 MB)
    assert 0.95 < fam["hbm_bytes_per_launch"] / 122.55e6 < 1.10
    assert t["scenes_per_launch"] == 4


def test_committed_default_line_has_the_contract_keys():
    d = json.load(open(os.path.join(REPO, "profiles", "r4_bench_default.json")))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["metric"] == "scenes/sec" and d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "f32" and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert r["frac"] == pytest.approx(r["achieved"] / r["peak"], rel=1e-9)
    assert r["achieved"] == pytest.approx(r["algorithmic_bytes_per_launch"] / (r["avg_launch_ms"] * 1e-3) / 1e9, rel=1e-6)
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["unit"] == "scenes/sec" and "sample" in c
    assert d["value"] == pytest.approx(d["total_scenes"] / (d["ms_per_step"] * 1e-3 * d["steps"]), rel=1e-6)


def test_dump_outputs_is_float32_within_budget_and_samples_the_same_elements(tmp_path):
    b = _bench()
    big = torch.arange(b.DUMP_MAX_VALUES + 12345, dtype=torch.float64)       # more values than one array's share
    small = torch.arange(10, dtype=torch.float32).reshape(2, 5)
    for run in ("a", "b"):
        b.dump_outputs(str(tmp_path / run), {"big": big, "small": small})
    got = {run: {n: np.load(tmp_path / run / f"{n}.npy") for n in ("big", "small")} for run in ("a", "b")}
    a = got["a"]
    assert a["big"].dtype == np.float32 and a["small"].dtype == np.float32
    assert a["big"].size == b.DUMP_MAX_VALUES // 2
    assert np.all(np.diff(a["big"]) > 0)                                      # distinct positions, in order
    np.testing.assert_array_equal(a["small"], np.arange(10, dtype=np.float32))
    for n in ("big", "small"):
        np.testing.assert_array_equal(a[n], got["b"][n])
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 * 2 ** 20


@pytest.mark.gpu
def test_plain_run_times_exactly_the_given_steps_and_dumps_the_last_step(tmp_path):
    steps = 3
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--workload", "shipped", "--steps", str(steps), "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    cfg = d["config"]
    B, N, C, H, W = cfg["scenes_per_step"], cfg["agents"], cfg["C"], cfg["H"], cfg["W"]
    assert d["metric"] == "scenes/sec" and d["unit"] == "scenes/sec" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == steps and d["total_scenes"] == steps * B
    assert d["value"] == pytest.approx(d["total_scenes"] / (d["ms_per_step"] * 1e-3 * steps), rel=1e-6)
    for k in ("sustained", "latency_ms_one_scene", "roofline", "exact_fp32_mode", "cpu_baseline"):
        assert d[k] is None, k                                                # measured by --full only
    share = _bench().DUMP_MAX_VALUES // 2
    for name, size in (("fused", B * C * H * W), ("pred_feature", B * N * C * H * W)):
        a = np.load(tmp_path / f"{name}.npy")
        assert a.dtype == np.float32 and a.size == min(size, share), name
        assert np.isfinite(a).all() and a.std() > 0, name
