"""bench.py end to end on one GPU at a small size: a plain run reports the headline figures, leaves the --full ones
null and dumps what the last timed step computed; --full still adds the roofline and kernel-family figures."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--workload", "c2", "--batch", "4", "--warmup", "1"]


def _bench(*argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *argv], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_bench_times_the_steps_and_dumps_the_last_one(tmp_path):
    d = tmp_path / "out"
    j = _bench("--steps", "3", "--dump-outputs", str(d))
    assert j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["value"] > 0
    assert j["unit"] == "samples/s" and j["higher_is_better"] is True and j["dtype"] == "f32"
    assert j["roofline"] is None and j["roofline_fusion"] is None and j["kernel_families"] is None and j["cpu_baseline"] is None
    arrays = {p[:-4]: np.load(d / p) for p in os.listdir(d)}
    assert set(arrays) == {"loss", "pred_gaze", "preds", "img_feat", "initial_rot_feat", "feats", "grad_sample", "param_sample"}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64_000_000
    B, V, iters = 4, 2, 3
    assert arrays["pred_gaze"].shape == (B, 2) and arrays["preds"].shape == (iters, V * (V - 1), B, 2)
    assert arrays["img_feat"].shape[:2] == (V, B) and arrays["feats"].shape[:3] == (iters, V * (V - 1), B)
    np.testing.assert_array_equal(arrays["pred_gaze"], arrays["preds"][-1, 0])
    assert float(arrays["loss"].reshape(-1)[0]) == pytest.approx(j["config"]["loss"], rel=1e-6)


def test_full_bench_adds_the_secondary_figures():
    j = _bench("--steps", "2", "--full", "--no-cpu-baseline")
    assert j["steps"] == 2 and j["ms_per_step"] > 0
    assert j["roofline"]["achieved"] > 0 and j["roofline"]["launches_per_step"] > 0
    assert j["kernel_families"]
