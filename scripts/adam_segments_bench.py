#!/usr/bin/env python3
"""The segmented Adam step (mvg_adam_step_segments) against the one-launch step (mvg_adam_step) on the ResNet-50 model's arena:
  full           mvg_adam_step over the whole arena (the parent's kernel: the yardstick)
  seg_full       one segment over the whole arena
  seg_head       the head-only step: heads, fusers and lifter in one segment
  seg_l34_head   layer3 + layer4 at one learning rate and the head at another: two segments
  dev_full, dev_head, dev_l34_head   the same three plans through mvg_adam_step_segments_dev: learning rates and step counters
                 on the device, a one-block launch that advances the counters in front of every update (the captured step's form)
Device events around CALLS back-to-back launches, ROUNDS rounds that alternate the seven, the median over rounds and the
round-to-round spread (min .. max) per variant; GB/s on 28 B per active element.  Synthetic values.
Usage: adam_segments_bench.py [--calls 20] [--rounds 5] [--out FILE.json]"""
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
HEAD = (1e-3, 0.9, 0.999, 1e-8, 0.0)
BODY = (1e-4, 0.9, 0.999, 1e-8, 1e-6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    m = MultiViewGaze(50, 3).to(dev)
    m.ensure_layout()
    _, entries = m.grad_arena()
    names = {id(p): k for k, p in m.named_parameters()}
    n = m.param_arena().numel()
    lay = [(off, cnt) for (_, off, cnt) in entries]
    is_bb = [names[id(p)].startswith("_feat_extractor") for (p, _, _) in entries]
    is_l34 = [".layer3." in names[id(p)] or ".layer4." in names[id(p)] for (p, _, _) in entries]
    ones = [1] * len(lay)

    def records(group_of, has):
        return [(s.begin, s.end) + s.group + (s.step,) for s in plan_segments(lay, group_of, has, ones)]
    variants = {
        "seg_full": records([BODY] * len(lay), [True] * len(lay)),
        "seg_head": records([HEAD] * len(lay), [not b for b in is_bb]),
        "seg_l34_head": records([BODY if b else HEAD for b in is_bb], [(not b) or l for b, l in zip(is_bb, is_l34)]),
    }
    assert [len(v) for v in variants.values()] == [1, 1, 2] and variants["seg_full"][0][:2] == (0, n)
    g = torch.Generator().manual_seed(0)
    p = torch.randn(n, generator=g).to(dev)
    gr = (torch.randn(n, generator=g) * 0.01).to(dev)
    mo, ve = torch.zeros(n, device=dev), torch.zeros(n, device=dev)

    runs = {"full": lambda: ops.adam_step(p, gr, mo, ve, *BODY, 1)}
    for k, segs in variants.items():
        runs[k] = (lambda s: lambda: ops.adam_step_segments(p, gr, mo, ve, s))(segs)
    active = {"full": n, **{k: sum(e - b for b, e, *_ in segs) for k, segs in variants.items()}}
    lr_dev = torch.tensor([HEAD[0], BODY[0]], dtype=torch.float32).to(dev)
    for k, segs in variants.items():                      # (begin, end, lr index, betas, eps, weight_decay) and one zeroed row per segment
        recs = [(b, e, 0 if lr == HEAD[0] else 1, b1, b2, eps, wd) for (b, e, lr, b1, b2, eps, wd, _) in segs]
        rows = torch.zeros(len(recs), 3, device=dev)
        runs["dev" + k[3:]] = (lambda s, r: lambda: ops.adam_step_segments_dev(p, gr, mo, ve, s, lr_dev, r))(recs, rows)
        active["dev" + k[3:]] = active[k]
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
    out = {"device": torch.cuda.get_device_name(0), "arena_elements": n, "calls_per_round": a.calls, "rounds": a.rounds, "variants": {}}
    for k, ts in per_call.items():
        med = float(np.median(ts))
        out["variants"][k] = {"segments": len(variants.get("seg" + k[3:], [])), "active_elements": active[k],
                              "ms_per_call_median": round(med, 4), "ms_per_call_min": round(min(ts), 4),
                              "ms_per_call_max": round(max(ts), 4), "GBps_on_28B_per_active_element": round(28.0 * active[k] / med / 1e6, 1)}
        print(k, json.dumps(out["variants"][k]), flush=True)
    full = out["variants"]["full"]["ms_per_call_median"]
    out["over_full"] = {k: round(v["ms_per_call_median"] / full, 4) for k, v in out["variants"].items()}
    out["active_share"] = {k: round(active[k] / n, 4) for k in runs}
    out["dev_over_seg"] = {k[4:]: round(out["variants"][k]["ms_per_call_median"] / out["variants"]["seg" + k[3:]]["ms_per_call_median"], 4)
                           for k in runs if k.startswith("dev_")}
    print(json.dumps({"over_full": out["over_full"], "active_share": out["active_share"], "dev_over_seg": out["dev_over_seg"]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
