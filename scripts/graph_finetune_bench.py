#!/usr/bin/env python3
"""The fine-tuning step captured in a hipGraph against the eager fine-tuning step, ResNet-50, two parameter groups
({backbone} lr 1e-4, weight_decay 1e-6; {head} lr 1e-3), two configurations:
  frozen_stem_layer1_layer2   layer3 + layer4 + head train (the configuration of finetune_step_bench.py)
  head_only                   the whole backbone frozen
and three arms per configuration, in ONE process, ROUNDS rounds that alternate the three:
  eager_overlap      the eager step, overlap_wgrad on, optim.Adam(capturable=False)
  eager_no_overlap   the eager step, overlap_wgrad off, optim.Adam(capturable=False)
  captured           graph.GraphedStep over optim.Adam(capturable="segments") (single-stream capture), one replay per step
The eager arms share one model (the flag is flipped between rounds), the captured arm has a twin of its own (a capture pins its
buffers).  Per round and arm: one untimed step, then STEPS steps under a host clock - `host` stops when the last step is queued,
`wall` after the device synchronise that follows - and a pair of device events.  Medians and min .. max over rounds.
Synthetic weights and inputs.
Usage: graph_finetune_bench.py [--views 4] [--batch 32] [--hw 224] [--steps 20] [--rounds 5] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import rot_mvgaze_amd  # noqa: E402,F401
from rot_mvgaze_amd import synth  # noqa: E402
from rot_mvgaze_amd.geometry import rotation_matrix_2d  # noqa: E402
from rot_mvgaze_amd.graph import GraphedStep  # noqa: E402
from rot_mvgaze_amd.losses import MultiViewIterationLoss  # noqa: E402
from rot_mvgaze_amd.model import MultiViewGaze  # noqa: E402
from rot_mvgaze_amd.optim import Adam  # noqa: E402

dev = torch.device("cuda:0")
FROZEN = {
    "frozen_stem_layer1_layer2": lambda k: k.startswith("_feat_extractor") and ".layer3." not in k and ".layer4." not in k,
    "head_only": lambda k: k.startswith("_feat_extractor"),
}


def build(weights, frozen, capturable, img, rot, gt):
    m = MultiViewGaze(50, 3)
    m.load_state_dict(weights, strict=True)
    m.to(dev).train()
    named = dict(m.named_parameters())
    for k, p in named.items():
        if frozen(k):
            p.requires_grad_(False)
    opt = Adam([{"params": [p for k, p in named.items() if k.startswith("_feat_extractor")], "lr": 1e-4, "weight_decay": 1e-6},
                {"params": [p for k, p in named.items() if not k.startswith("_feat_extractor")], "lr": 1e-3, "weight_decay": 0.0}],
               capturable=capturable)
    crit = MultiViewIterationLoss(rel_weight=0.01, reference_decay=1.0, iter_decay=0.5)

    def step():
        m.zero_grad(set_to_none=True)
        loss = crit(m.forward_multiview(img, rot), gt)
        loss.backward()
        opt.step()
        return loss
    return m, opt, step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    V, B = a.views, a.batch
    weights = {k: torch.from_numpy(np.array(v)) for k, v in synth.make_state_dict(50, 0, 3).items()}
    inp = synth.make_inputs(B, V, 1234, a.hw)
    img = [torch.from_numpy(np.ascontiguousarray(inp["img"][:, v])).to(dev) for v in range(V)]
    gt = torch.from_numpy(inp["gt_gaze"]).to(dev)
    rot = rotation_matrix_2d(torch.from_numpy(inp["head_pose"]).reshape(-1, 2).to(dev)).reshape(B, V, 3, 3)
    out = {"device": torch.cuda.get_device_name(0), "model": "ResNet-50", "views": V, "batch": B, "input": f"3x{a.hw}x{a.hw} fp32",
           "steps_per_round": a.steps, "rounds": a.rounds, "configurations": {}}
    for config, frozen in FROZEN.items():
        me, _, eager = build(weights, frozen, False, img, rot, gt)
        mg, og, graphed = build(weights, frozen, "segments", img, rot, gt)
        for flag in (True, False):                         # warm-up of both eager forms
            me.ensure_layout()
            me._backbone.overlap_wgrad = flag
            for _ in range(2):
                eager()
        gs = GraphedStep(mg, graphed, og, warmup=3)
        gs.run()
        torch.cuda.synchronize()

        def arm(name):
            if name == "captured":
                return gs.run
            me._backbone.overlap_wgrad = name == "eager_overlap"
            return eager
        ms = {name: {"wall": [], "host": [], "device": []} for name in ("eager_overlap", "eager_no_overlap", "captured")}
        for _ in range(a.rounds):
            for name in ms:
                fn = arm(name)
                fn()                                       # (the first step after a switch: not timed)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                for _ in range(a.steps):
                    fn()
                e1.record()
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                ms[name]["host"].append((t1 - t0) * 1e3 / a.steps)
                ms[name]["wall"].append((t2 - t0) * 1e3 / a.steps)
                ms[name]["device"].append(e0.elapsed_time(e1) / a.steps)
        res = {}
        for name, d in ms.items():
            res[name] = {f"{what}_ms_per_step_{stat}": round(float(f(ts)), 3) for what, ts in d.items()
                         for stat, f in (("median", np.median), ("min", min), ("max", max))}
            print(config, name, json.dumps(res[name]), flush=True)
        res["captured_over_eager_overlap_wall"] = round(res["captured"]["wall_ms_per_step_median"] / res["eager_overlap"]["wall_ms_per_step_median"], 4)
        res["captured_over_eager_no_overlap_wall"] = round(res["captured"]["wall_ms_per_step_median"] /
                                                           res["eager_no_overlap"]["wall_ms_per_step_median"], 4)
        res["host_ms_freed_per_step"] = round(res["eager_overlap"]["host_ms_per_step_median"] - res["captured"]["host_ms_per_step_median"], 3)
        print(config, json.dumps({k: v for k, v in res.items() if not isinstance(v, dict)}), flush=True)
        out["configurations"][config] = res
        del gs, me, mg, og, eager, graphed
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f_:
            json.dump(out, f_, indent=1)


if __name__ == "__main__":
    main()
