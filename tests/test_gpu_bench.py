"""GPU: bench.py end to end on a small tile.  A plain run prints the headline line and runs no other leg; `--full` adds the other
2D legs (the 3D and sharded legs are left out here for time)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("value_host_input", "nms2d_strict", "exact_f32", "split_bf16x6", "cpu_baseline", "sharded_2d", "value_3d", "sharded_3d")


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--size", "512", "--steps", "2", "--warmup", "1"] + list(args),
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_only(tmp_path):
    out = _bench("--dump-outputs", str(tmp_path))
    for k in HEADLINE:
        assert k in out, k
    assert out["unit"] == "Mpix/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["value"] > 0 and out["steps"] == 2 and out["warmup"] == 1
    assert out["value"] == pytest.approx(512 * 512 / (out["ms_per_step"] * 1e-3) / 1e6, rel=1e-2)
    assert out["full"] is False
    assert "stages_ms" in out and "roofline" in out
    for k in FULL_ONLY:
        assert k not in out, k
    labels = np.load(tmp_path / "labels.npy")
    assert labels.shape == (512, 512) and labels.max() > 0 and out["config"]["survivors"] > 0
    assert sorted(out["dump_outputs"]["arrays"]) == ["labels", "res_coord", "res_points", "res_prob"]


def test_full_run_adds_the_other_legs():
    out = _bench("--full", "--skip-3d", "--no-sharded", "--no-cpu-baseline")
    assert out["full"] is True and out["value"] > 0
    assert out["config"]["candidates"] > 0
    assert out["nms2d_strict"]["value"] > 0
    assert out["value_host_input"]["value"] > 0
    assert out["exact_f32"]["value"] > 0 and out["split_bf16x6"]["value"] > 0
    for k in ("cpu_baseline", "sharded_2d", "value_3d"):
        assert k not in out, k
