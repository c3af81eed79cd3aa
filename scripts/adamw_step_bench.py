#!/usr/bin/env python3
"""Decoupled weight decay against the coupled step it sits next to, on the ResNet-50 model's arena, in one process:
  adam_step      mvg_adam_step over the whole arena (the parent's kernel, unchanged: the yardstick)
  adamw_step     mvg_adamw_step over the whole arena
  seg_l34_head   mvg_adam_step_segments: layer3 + layer4 at one learning rate and the head at another (two coupled segments)
  ex_l34_head    mvg_adam_step_segments_ex over the same two segments, the backbone's coupled and the head's decoupled
Device events around CALLS back-to-back launches, ROUNDS rounds that alternate the four, the median over rounds and the
round-to-round spread (min .. max) per variant; GB/s on 28 B per active element.  Synthetic values.
Usage: adamw_step_bench.py [--calls 200] [--rounds 7] [--out FILE.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import rot_mvgaze_amd  # noqa: E402,F401
from rot_mvgaze_amd import ops  # noqa: E402
from rot_mvgaze_amd.model import MultiViewGaze  # noqa: E402
from rot_mvgaze_amd.optim import plan_segments  # noqa: E402

dev = torch.device("cuda:0")
HEAD = (1e-3, 0.9, 0.999, 1e-8, 1e-2)
BODY = (1e-4, 0.9, 0.999, 1e-8, 1e-6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.rounds >= 5
    m = MultiViewGaze(50, 3).to(dev)
    m.ensure_layout()
    _, entries = m.grad_arena()
    names = {id(p): k for k, p in m.named_parameters()}
    n = m.param_arena().numel()
    lay = [(off, cnt) for (_, off, cnt) in entries]
    is_bb = [names[id(p)].startswith("_feat_extractor") for (p, _, _) in entries]
    is_l34 = [".layer3." in names[id(p)] or ".layer4." in names[id(p)] for (p, _, _) in entries]
    segs = plan_segments(lay, [BODY if b else HEAD for b in is_bb], [(not b) or l for b, l in zip(is_bb, is_l34)], [1] * len(lay))
    coupled = [(s.begin, s.end) + s.group + (s.step,) for s in segs]
    mixed = [r + (int(r[2:7] == HEAD),) for r in coupled]
    assert len(segs) == 2 and sorted(r[8] for r in mixed) == [0, 1]
    g = torch.Generator().manual_seed(0)
    p = torch.randn(n, generator=g).to(dev)
    gr = (torch.randn(n, generator=g) * 0.01).to(dev)
    mo, ve = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    runs = {"adam_step": lambda: ops.adam_step(p, gr, mo, ve, *HEAD, 1),
            "adamw_step": lambda: ops.adamw_step(p, gr, mo, ve, *HEAD, 1),
            "seg_l34_head": lambda: ops.adam_step_segments(p, gr, mo, ve, coupled),
            "ex_l34_head": lambda: ops.adam_step_segments_ex(p, gr, mo, ve, mixed)}
    part = sum(s.end - s.begin for s in segs)
    active = {"adam_step": n, "adamw_step": n, "seg_l34_head": part, "ex_l34_head": part}
    for fn in runs.values():                              # every variant once: code objects loaded, caches in their steady state
        fn()
    torch.cuda.synchronize()
    per_call = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.calls):
                fn()
            t1.record()
            t1.synchronize()
            per_call[k].append(t0.elapsed_time(t1) / a.calls)
    assert bool(torch.isfinite(p).all())
    out = {"device": torch.cuda.get_device_name(0), "arena_elements": n, "calls_per_round": a.calls, "rounds": a.rounds, "variants": {}}
    for k, ts in per_call.items():
        med = float(np.median(ts))
        out["variants"][k] = {"active_elements": active[k], "ms_per_call_median": round(med, 4), "ms_per_call_min": round(min(ts), 4),
                              "ms_per_call_max": round(max(ts), 4), "ms_per_call_rounds": [round(t, 4) for t in ts],
                              "GBps_on_28B_per_active_element": round(28.0 * active[k] / med / 1e6, 1)}
        print(k, json.dumps(out["variants"][k]), flush=True)
    v = out["variants"]
    out["adamw_over_adam"] = round(v["adamw_step"]["ms_per_call_median"] / v["adam_step"]["ms_per_call_median"], 4)
    out["ex_over_segments"] = round(v["ex_l34_head"]["ms_per_call_median"] / v["seg_l34_head"]["ms_per_call_median"], 4)
    out["adamw_inside_adam_spread"] = bool(v["adam_step"]["ms_per_call_min"] <= v["adamw_step"]["ms_per_call_median"]
                                           <= v["adam_step"]["ms_per_call_max"])
    print(json.dumps({k: out[k] for k in ("adamw_over_adam", "ex_over_segments", "adamw_inside_adam_spread")}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
