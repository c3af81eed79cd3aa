#!/usr/bin/env python3
"""The evaluation loop's metric, two ways, on one eval-mode forward per batch (ResNet-18, V=2, B=64, 224 px, synthetic weights
and inputs; the batches are one static batch: data loading is not what is measured):
  (a) reference  the reference trainer's test loop (trainer.py:169-192): per batch pred.cpu().numpy() / gt.cpu().numpy() into
                 float64 host arrays, the host metric geometry.angular_error over them after the last batch;
  (b) meter      metrics.AngularErrorMeter.update per batch and ONE compute() after the last batch.
Per loop: wall time per batch (perf_counter around the whole loop, which ends in a device synchronise) and the host time spent
blocked in the device-to-host copies (perf_counter around each .cpu() call, or around compute()).  The two loops alternate,
--repeats times each, after a warm-up of both; every run is kept.  Also measured here, on the shapes of
tests/test_gaze_error_gpu.py: the largest |device - float64 host metric| per element on the double path (single-row updates).
Usage: eval_metric_bench.py [--batches N] [--warmup W] [--repeats R] [--out profiles/gaze_error_meter.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gaze_error_ref as R  # noqa: E402
import rot_mvgaze_amd  # noqa: E402,F401
from rot_mvgaze_amd import ops, synth  # noqa: E402
from rot_mvgaze_amd.geometry import angular_error, rotation_matrix_2d  # noqa: E402
from rot_mvgaze_amd.metrics import AngularErrorMeter  # noqa: E402
from rot_mvgaze_amd.model import FeatRotationSymm  # noqa: E402

dev = torch.device("cuda:0")
DEPTH, V, B, HW, ITERS = 18, 2, 64, 224, 3


def per_element_max():
    """max |device - oracle| in degrees over the rows >= R.FLOOR_DEG of every test shape (the double path: one row per update)."""
    worst, rows, below = 0.0, 0, 0
    for I, D, n in R.SHAPES:
        preds, gt = R.make_inputs(I, D, n, seed=7)
        want = R.oracle_cells(preds, gt)
        p, g = torch.from_numpy(preds).to(dev), torch.from_numpy(gt).to(dev)
        recs = torch.zeros(n, I, D, 5, dtype=torch.float64, device=dev)
        for b in range(n):
            ops.gaze_error_update(p[:, :, b:b + 1].contiguous(), g[:, b:b + 1].contiguous(), I, D, 1, recs[b])
        got = np.moveaxis(recs.cpu().numpy()[..., 1], 0, -1)
        held = want >= R.FLOOR_DEG
        worst = max(worst, float(np.abs(got - want)[held].max()))
        rows, below = rows + int(held.sum()), below + int((~held).sum())
    return {"max_abs_deviation_deg": worst, "rows_held": rows, "rows_below_floor": below, "floor_deg": R.FLOOR_DEG,
            "bar_deg": R.PER_ELEMENT_BAR_DEG, "oracle": "geometry.angular_error on float64, similarity clamped to [-1, 1]"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaze_error_meter.json"))
    a = ap.parse_args()
    m = FeatRotationSymm(DEPTH, ITERS)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.make_state_dict(DEPTH, 0, ITERS, perturb_bn=True).items()},
                      strict=True)
    m.to(dev).eval()
    inp = synth.make_inputs(B, V, 1234, HW)
    img, hp, gt = (torch.from_numpy(inp[k]) for k in ("img", "head_pose", "gt_gaze"))
    base = {"img_0": img[:, 0].contiguous().to(dev), "img_1": img[:, 1].contiguous().to(dev),
            "rot_0": rotation_matrix_2d(hp[:, 0].contiguous().to(dev)), "rot_1": rotation_matrix_2d(hp[:, 1].contiguous().to(dev)),
            "gt_gaze": gt[:, 0].contiguous().to(dev), "gt_gaze_1": gt[:, 1].contiguous().to(dev)}
    meter = AngularErrorMeter(num_iter=ITERS, dirs=2, device=dev, output_index=m._output_index)

    def reference_loop(n):
        pred_all, gt_all, blocked = np.zeros((n * B, 2)), np.zeros((n * B, 2)), 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            for k in range(n):
                data = m(dict(base))
                c0 = time.perf_counter()
                pred, lab = data["pred_gaze"].cpu(), data["gt_gaze"].cpu()
                blocked += time.perf_counter() - c0
                pred_all[k * B:(k + 1) * B], gt_all[k * B:(k + 1) * B] = pred.numpy(), lab.numpy()
        error = float(np.mean(angular_error(pred_all, gt_all)))
        torch.cuda.synchronize()
        return time.perf_counter() - t0, blocked, error

    def meter_loop(n):
        meter.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            for _ in range(n):
                meter.update(m(dict(base)))
        c0 = time.perf_counter()
        error = meter.compute()["error_gaze"]
        blocked = time.perf_counter() - c0
        torch.cuda.synchronize()
        return time.perf_counter() - t0, blocked, error

    reference_loop(a.warmup)
    meter_loop(a.warmup)
    runs = {"reference": [], "meter": []}
    for _ in range(a.repeats):
        for name, fn in (("reference", reference_loop), ("meter", meter_loop)):
            wall, blocked, error = fn(a.batches)
            runs[name].append({"wall_ms_per_batch": round(1e3 * wall / a.batches, 4), "host_blocked_in_copy_ms_per_batch":
                               round(1e3 * blocked / a.batches, 4), "error_gaze_deg": error})
    out = {"device": torch.cuda.get_device_name(0),
           "shape": {"depth": DEPTH, "views": V, "batch": B, "hw": HW, "num_iter": ITERS, "batches": a.batches, "warmup": a.warmup},
           "loops": {k: {"wall_ms_per_batch_median": statistics.median(r["wall_ms_per_batch"] for r in v),
                         "host_blocked_in_copy_ms_per_batch_median": statistics.median(r["host_blocked_in_copy_ms_per_batch"] for r in v),
                         "runs": v} for k, v in runs.items()},
           "error_gaze_abs_difference_deg": abs(runs["reference"][-1]["error_gaze_deg"] - runs["meter"][-1]["error_gaze_deg"]),
           "per_element": per_element_max()}
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
