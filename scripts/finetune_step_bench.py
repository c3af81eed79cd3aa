#!/usr/bin/env python3
"""One ResNet-50 training step (zero_grad + forward + loss + backward + Adam) with the stem, layer1 and layer2 frozen against the
same step with everything trainable, on ONE model: requires_grad is flipped between rounds (nothing is rebuilt).  Two parameter
groups in both forms ({backbone} lr 1e-4, weight_decay 1e-6; {head} lr 1e-3): the frozen form steps the segments of
layer3 + layer4 + head, the unfrozen form the whole arena in two or three segments (the prefix keeps a step count of its own once
it sat out a round).  Device events around STEPS steps, ROUNDS rounds that
alternate the two forms, medians and round-to-round spread; the bytes the forward leaves allocated for the backward.
Synthetic weights and inputs.
Usage: finetune_step_bench.py [--views 4] [--batch 32] [--steps 5] [--rounds 5] [--out FILE.json]"""
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
from rot_mvgaze_amd.optim import Adam  # noqa: E402

dev = torch.device("cuda:0")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    V, B = a.views, a.batch
    m = MultiViewGaze(50, 3)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.make_state_dict(50, 0, 3).items()}, strict=True)
    m.to(dev).train()
    inp = synth.make_inputs(B, V, 1234, 224)
    img = [torch.from_numpy(np.ascontiguousarray(inp["img"][:, v])).to(dev) for v in range(V)]
    gt = torch.from_numpy(inp["gt_gaze"]).to(dev)
    rot = rotation_matrix_2d(torch.from_numpy(inp["head_pose"]).reshape(-1, 2).to(dev)).reshape(B, V, 3, 3)
    crit = MultiViewIterationLoss(rel_weight=0.01, reference_decay=1.0, iter_decay=0.5)
    named = dict(m.named_parameters())
    prefix = [p for k, p in named.items() if k.startswith("_feat_extractor") and ".layer3." not in k and ".layer4." not in k]
    opt = Adam([{"params": [p for k, p in named.items() if k.startswith("_feat_extractor")], "lr": 1e-4, "weight_decay": 1e-6},
                {"params": [p for k, p in named.items() if not k.startswith("_feat_extractor")], "lr": 1e-3, "weight_decay": 0.0}])
    held = {}

    def step(form):
        opt.zero_grad()
        before = torch.cuda.memory_allocated()
        loss = crit(m.forward_multiview(img, rot), gt)
        held[form] = torch.cuda.memory_allocated() - before
        loss.backward()
        opt.step()

    def set_form(form):
        for p in prefix:
            p.requires_grad_(form == "unfrozen")
    ms = {"unfrozen": [], "frozen_stem_layer1_layer2": []}
    for form in ms:                                       # warm-up of both forms
        set_form(form)
        for _ in range(2):
            step(form)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for form in ms:
            set_form(form)
            step(form)                                    # (the first step after a flip: not timed)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                step(form)
            t1.record()
            t1.synchronize()
            ms[form].append(t0.elapsed_time(t1) / a.steps)
    out = {"device": torch.cuda.get_device_name(0), "model": "ResNet-50", "views": V, "batch": B, "input": "3x224x224 fp32",
           "steps_per_round": a.steps, "rounds": a.rounds, "forms": {}}
    for form, ts in ms.items():
        out["forms"][form] = {"ms_per_step_median": round(float(np.median(ts)), 3), "ms_per_step_min": round(min(ts), 3),
                              "ms_per_step_max": round(max(ts), 3), "forward_bytes_held_for_backward": int(held[form])}
        print(form, json.dumps(out["forms"][form]), flush=True)
    f, u = out["forms"]["frozen_stem_layer1_layer2"], out["forms"]["unfrozen"]
    out["frozen_over_unfrozen_step"] = round(f["ms_per_step_median"] / u["ms_per_step_median"], 4)
    out["frozen_over_unfrozen_bytes_held"] = round(f["forward_bytes_held_for_backward"] / u["forward_bytes_held_for_backward"], 4)
    print(json.dumps({k: out[k] for k in ("frozen_over_unfrozen_step", "frozen_over_unfrozen_bytes_held")}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f_:
            json.dump(out, f_, indent=1)


if __name__ == "__main__":
    main()
