"""GPU (one MI355X): a plain `bench.py` run times the headline step only, and `--dump-outputs` writes what the last timed step returned --
the same values from two runs with the same arguments, so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--small", "--dump-outputs", out_dir]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])


def test_plain_run_and_reproducible_dumped_outputs(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    d = _bench(a)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0, d
    assert abs(d["value"] - d["config"]["images_per_gpu_per_step"] * 1e3 / d["ms_per_step"]) <= 1e-6 * d["value"], d
    assert not {"roofline", "fwd_only", "launches_per_micro_step", "batch_24", "accum_fused", "window_towers", "cpu_baseline"} & set(d), sorted(d)
    names = sorted(os.listdir(a))
    assert names == ["align_loss.npy", "ce_loss.npy", "loss.npy", "regression_loss.npy"], names
    assert float(np.load(os.path.join(a, "loss.npy"))) == d["loss"]
    _bench(b)
    for n in names:
        x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        assert x.dtype == np.float32 and np.isfinite(x).all(), (n, x)
        assert np.array_equal(x, y), (n, x, y)
