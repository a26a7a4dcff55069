"""bench.py end to end on the GPU (the benchmark itself is what these tests are about, so each
starts it once as a child process, at the default workload: the roofline figures need the
256-image shapes that route to the dominant GEMM kernel).

A plain run times exactly --steps steps and prints the headline line without the figures that
take runs of their own; --full brings those back; --dump-outputs writes the last timed step's
outputs. The CPU baseline (up to 60 s of host time) is left out here with --no-cpu-baseline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"}
FULL_ONLY = {"roofline", "library_gemm", "train_transform", "cpu_baseline"}


def run_bench(*argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--steps", "2", "--warmup", "1", *argv],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_outputs(dev, tmp_path):
    out = tmp_path / "dump"
    d = run_bench("--dump-outputs", str(out))
    assert HEADLINE <= set(d) and not FULL_ONLY & set(d)
    assert d["steps"] == 2 and d["warmup"] == 1 and d["dtype"] == "bf16"
    assert d["unit"] == "images/s" and d["higher_is_better"] is True
    # value and ms_per_step are the same measurement: 256 images per step on one GPU
    assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] / 1e3 / 256 - 1) < 1e-3
    assert d["image_tower"]["source"] == "timed loop"
    assert sorted(os.listdir(out)) == ["loss.npy", "probs.npy"]
    loss, probs = np.load(out / "loss.npy"), np.load(out / "probs.npy")
    assert loss.dtype == probs.dtype == np.float32
    assert loss.size == 1 and probs.shape == (256, 10)
    assert np.isfinite(loss).all() and np.isfinite(probs).all()
    assert np.abs(probs.sum(1) - 1).max() < 1e-5  # f32 softmax rows over 10 classes


@pytest.mark.gpu
def test_full_run_restores_the_other_figures(dev):
    d = run_bench("--full", "--no-cpu-baseline")
    assert HEADLINE <= set(d) and d["steps"] == 2
    assert FULL_ONLY - {"cpu_baseline"} <= set(d) and "cpu_baseline" not in d
    assert d["roofline"]["launches_per_step"] > 0 and 0 < d["roofline"]["frac"] < 1
    assert d["library_gemm"]["launches_per_step"] >= 1
    assert d["train_transform"]["avg_launch_us"] > 0
