#!/usr/bin/env python3
"""Frozen-BatchNorm training steps (model.train() + model.freeze_batchnorm) of the fp32 model with model.split_frozen off - the
fp32-MFMA kernels: bit for bit the step as it was before the flag existed, so it is the baseline - and on - the split-operand
kernels with activation scales from the conv launches' statistics partials.  Each is measured twice, alternating (off, on, off,
on): the spread between the baseline's own two runs is what a difference has to exceed.  Median of event-timed steps after a
warm-up, one process, synthetic weights and inputs (the scheme of frozen_step_bench.py).  The train-mode step on the split
kernels is timed last, for scale (it moves the running statistics).
Usage: frozen_split_bench.py [--steps K] [--warmup W] [--out FILE.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import rot_mvgaze_amd  # noqa: E402,F401
from rot_mvgaze_amd import synth  # noqa: E402
from rot_mvgaze_amd.geometry import rotation_matrix_2d  # noqa: E402
from rot_mvgaze_amd.losses import MultiViewIterationLoss  # noqa: E402
from rot_mvgaze_amd.model import MultiViewGaze  # noqa: E402

dev = torch.device("cuda:0")
CASES = [("R18 V=2 B=64 224px", 18, 2, 64, 224), ("R50 V=4 B=32 224px", 50, 4, 32, 224)]


def event_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def model_case(depth, V, B, hw, steps, warmup):
    m = MultiViewGaze(depth, 3)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.make_state_dict(depth, 0, 3).items()})
    m.to(dev).train()
    m.freeze_batchnorm = True
    inp = synth.make_inputs(B, V, 1234, hw)
    img = [torch.from_numpy(inp["img"][:, v]).contiguous().to(dev) for v in range(V)]
    rot = rotation_matrix_2d(torch.from_numpy(inp["head_pose"]).reshape(-1, 2).to(dev)).reshape(B, V, 3, 3).contiguous()
    gt = torch.from_numpy(inp["gt_gaze"]).to(dev)
    crit = MultiViewIterationLoss(rel_weight=0.01, reference_decay=1.0, iter_decay=0.5)

    def step():
        m.zero_grad(set_to_none=False)
        crit(m.forward_multiview(img, rot), gt).backward()
    res = {"flag_off_ms": [], "flag_on_ms": [], "flag_off_min_ms": [], "flag_on_min_ms": []}
    for flag in (False, True, False, True):
        m.split_frozen = flag
        med, best = event_ms(step, steps, warmup)
        call = m._backbone._last_call
        assert call.sp == flag and not call.training and call.train_step, call._replace(wprep=None, act_sinv=None)
        key = "flag_on" if flag else "flag_off"
        res[key + "_ms"].append(round(med, 3))
        res[key + "_min_ms"].append(round(best, 3))
    off, on = res["flag_off_ms"], res["flag_on_ms"]
    res["baseline_spread_ms"] = round(abs(off[0] - off[1]), 3)
    res["on_over_off"] = round(float(np.mean(on)) / float(np.mean(off)), 3)
    res["faster_by_more_than_the_spread"] = bool(min(off) - max(on) > abs(off[0] - off[1]))
    m.freeze_batchnorm = False
    med, best = event_ms(step, steps, warmup)
    res["train_mode_split_ms"] = round(med, 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "cases": {}}
    for name, depth, V, B, hw in CASES:
        out["cases"][name] = model_case(depth, V, B, hw, a.steps, a.warmup)
        print(name, json.dumps(out["cases"][name]), flush=True)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
