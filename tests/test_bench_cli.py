"""bench.py's command line: a plain run measures the headline figure only, --full adds the rest,
--dump-outputs writes what the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def test_dump_outputs_writes_float_arrays(tmp_path):
    import bench
    boxes = np.arange(8, dtype=np.float64).reshape(2, 4)
    scores = np.array([0.5, 0.25], np.float32)
    bench.dump_outputs(str(tmp_path / "d"), {"boxes": boxes, "scores": scores}, rank=0, world=1)
    np.testing.assert_array_equal(np.load(tmp_path / "d" / "boxes.npy"), boxes)
    got = np.load(tmp_path / "d" / "scores.npy")
    assert got.dtype == np.float32 and np.array_equal(got, scores)
    # ranks past the first of a multi-GPU run write beside rank 0, not over it
    bench.dump_outputs(str(tmp_path / "d"), {"boxes": boxes + 1}, rank=1, world=2)
    np.testing.assert_array_equal(np.load(tmp_path / "d" / "boxes.npy"), boxes)
    np.testing.assert_array_equal(np.load(tmp_path / "d" / "boxes_rank1.npy"), boxes + 1)
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path / "d"), {"ids": np.arange(3)}, rank=0, world=1)


def _bench(*argv):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--batch", "2"] + list(argv),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return lines[0]


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    d = tmp_path / "out"
    line = _bench("--steps", "3", "--warmup", "2", "--dump-outputs", str(d))
    assert all(k in line for k in HEADLINE) and line["steps"] == 3
    assert line["value"] == pytest.approx(2 * 3 / (line["ms_per_step"] * 3 / 1e3), rel=1e-3)
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["host_frames_fps_rank0"] is None
    assert "extra_workloads" not in line
    boxes, scores = np.load(d / "boxes.npy"), np.load(d / "scores.npy")
    assert boxes.shape == (2, 4) and boxes.dtype == np.float64 and np.all(np.isfinite(boxes))
    assert scores.shape == (2,) and scores.dtype == np.float32 and np.all((scores >= 0) & (scores <= 1))


@pytest.mark.gpu
def test_full_run_adds_the_probe_and_host_frames():
    line = _bench("--steps", "3", "--warmup", "2", "--full", "--no-cpu-baseline", "--host-frames", "2")
    assert all(k in line for k in HEADLINE)
    assert line["roofline"]["classes"] and line["host_frames_fps_rank0"] > 0
