"""bench.py's plain run and --dump-outputs: the arrays the last timed step left, as float64 .npy
files within the size budget, and a line whose `steps` / `ms_per_step` / `viol` say what ran."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_dump_outputs_writes_float64_arrays(tmp_path):
    import bench

    arrays = {"P": np.arange(24, dtype=np.float32).reshape(1, 4, 6), "w": np.ones(6),
              "viol": np.array([2.5])}
    bench.dump_outputs(str(tmp_path), arrays)
    assert sorted(os.listdir(tmp_path)) == ["P.npy", "viol.npy", "w.npy"]
    for name, a in arrays.items():
        got = np.load(tmp_path / (name + ".npy"))
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got, a)


def test_dump_outputs_samples_past_the_budget_the_same_way_every_time(tmp_path, monkeypatch):
    import bench

    monkeypatch.setattr(bench, "DUMP_LIMIT", 64 << 10)
    big = np.random.RandomState(1).randn(100_000)
    small = np.arange(10.0)
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), {"y_pred": big, "viol": small})
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64 << 10
    a, b = np.load(tmp_path / "a" / "y_pred.npy"), np.load(tmp_path / "b" / "y_pred.npy")
    assert 0 < a.size < big.size
    np.testing.assert_array_equal(a, b)
    assert np.isin(a, big).all()
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "viol.npy"), small)


@pytest.mark.gpu
def test_plain_run_times_the_steps_it_is_given_and_dumps_the_last_one(tmp_path):
    """A small plain run: no profiled epoch, no CPU baseline, no extras; `steps` timed steps after
    `warmup` untimed ones; the dumped state has the workload's shapes."""
    n, d, k = 20_000, 2_000, 30
    env = dict(os.environ, SPFM_BENCH_N=str(n), SPFM_BENCH_D=str(d))
    out = tmp_path / "out"
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                         "--steps", "2", "--warmup", "1", "--dump-outputs", str(out)],
                        env=env, capture_output=True, text=True, timeout=600)
    assert pr.returncode == 0, pr.stderr[-3000:]
    lines = [ln for ln in pr.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, pr.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1
    assert line["metric"] == "pcd_epochs_per_sec" and line["unit"] == "epochs/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - 1e3 / line["ms_per_step"]) <= 1e-3 * line["value"] + 1e-3
    assert len(line["viol"]) == 3  # one warm-up step + two timed steps
    assert line["roofline"] is None and line["cpu_baseline"] is None
    assert "other_configs" not in line and "concurrent_fits" not in line
    shapes = {"P": (1, k, d), "w": (d,), "y_pred": (n,), "viol": (1,)}
    for name, shape in shapes.items():
        a = np.load(out / (name + ".npy"))
        assert a.dtype == np.float64 and a.shape == shape, (name, a.dtype, a.shape)
        assert np.isfinite(a).all(), name
    np.testing.assert_allclose(np.load(out / "viol.npy")[0], line["viol"][-1], rtol=1e-6,
                               atol=1e-6)
    P = np.load(out / "P.npy")
    assert abs(float((P != 0).mean()) - line["nonzero_frac_P_after"]) < 1e-3
