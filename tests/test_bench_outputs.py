"""bench.py's --dump-outputs and --full: the dump's format and sampling rule (CPU), and on the GPU that a plain run
prints the headline fields only, renders the same images in every run with the same arguments (whatever the
clock-dependent warmup ran), and that --full adds the roofline block."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _frame(n, seed):
    rng = np.random.default_rng(seed)
    return rng.random((n, 4), dtype=np.float32), rng.integers(0, 1 << 24, n, dtype=np.int64).astype(np.int32)


def test_dump_outputs_whole_frame(tmp_path):
    avg, rgb8 = _frame(77 * 33, 1)
    bench.dump_outputs(str(tmp_path / "d"), avg, rgb8)
    assert sorted(os.listdir(tmp_path / "d")) == ["avg.npy", "rgb8.npy"]
    a, r = np.load(tmp_path / "d" / "avg.npy"), np.load(tmp_path / "d" / "rgb8.npy")
    assert a.dtype == np.float32 and r.dtype == np.float32
    assert np.array_equal(a, avg) and np.array_equal(r.astype(np.int64), rgb8.astype(np.int64))


def test_dump_outputs_samples_a_frame_above_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 20 * 1000)
    monkeypatch.setattr(bench, "DUMP_SAMPLE_PIXELS", 700)
    avg, rgb8 = _frame(1001, 2)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), avg, rgb8)
    idx = np.load(tmp_path / "a" / "pixel_index.npy")
    assert idx.dtype == np.float64 and idx.shape == (700,) and np.all(np.diff(idx) > 0) and idx[-1] <= 1000
    i = idx.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "avg.npy"), avg[i])
    assert np.array_equal(np.load(tmp_path / "a" / "rgb8.npy").astype(np.int64), rgb8[i].astype(np.int64))
    assert np.array_equal(idx, np.load(tmp_path / "b" / "pixel_index.npy"))  # the same sample in every run
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 700 * 28 + 3 * 128


def test_a_whole_1080p_frame_fits_the_cap():
    assert 1920 * 1080 * 20 <= bench.DUMP_MAX_BYTES <= 64_000_000
    assert bench.DUMP_SAMPLE_PIXELS * 28 <= bench.DUMP_MAX_BYTES


SMALL = ["--gpus", "1", "--scene", "c3", "--width", "320", "--height", "180", "--steps", "3", "--warmup", "1",
         "--warmup-s", "0.05"]


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *args], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_is_lean_and_repeatable(tmp_path):
    outs = []
    for d in ("a", "b"):
        line = _bench("--dump-outputs", str(tmp_path / d))
        assert all(k in line for k in HEADLINE) and line["steps"] == 3
        assert "roofline" not in line and "cpu_baseline" not in line
        assert line["ms_per_step"] > 0 and line["value"] > 0
        outs.append({f: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    assert list(outs[0]) == ["avg.npy", "rgb8.npy"]
    assert outs[0]["avg.npy"].shape == (320 * 180, 4) and outs[0]["avg.npy"].max() > 0
    for f in outs[0]:
        assert np.array_equal(outs[0][f], outs[1][f]), f


@pytest.mark.gpu
def test_full_run_adds_the_roofline_block():
    line = _bench("--full", "--no-cpu-baseline")
    assert all(k in line for k in HEADLINE)
    assert line["roofline"]["kernel"] == "k_trace2" and line["roofline"]["launch_ms"] > 0
    assert "cpu_baseline" not in line
