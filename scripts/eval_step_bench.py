#!/usr/bin/env python3
"""One eval-mode gradient step (model.eval(), forward + loss + backward: BatchNorm on its running statistics, the one-pass
backward of bn.hip) against one train-mode step on the same conv family (MVG_SPLIT=0: the fp32-MFMA kernels), plus the
event-timed BatchNorm-backward family (bn_bwd_reduce + bn_bwd_apply; the eval pass is counted under bn_bwd_apply) and the
streaming rate of the BatchNorm-backward passes per ResNet-50 shape.  Synthetic weights and inputs.
Usage: eval_step_bench.py [--steps K] [--warmup W] [--out FILE.json]"""
import argparse
import json
import os
import sys

os.environ["MVG_SPLIT"] = "0"          # both modes on the fp32-MFMA conv kernels (before the package is imported)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import rot_mvgaze_amd  # noqa: E402,F401
from rot_mvgaze_amd import ops, synth  # noqa: E402
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


def bn_family(fn):
    torch.cuda.synchronize()
    ops.prof_reset()
    ops.prof_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        fam = ops.prof_collect()
    finally:
        ops.prof_enable(False)
    out = {}
    for k in ("bn_bwd_reduce", "bn_bwd_apply"):
        e = fam.get(k, {"launches": 0, "ms": 0.0, "bytes": 0.0})
        out[k] = {"launches": e["launches"], "ms": round(e["ms"], 3), "GB": round(e["bytes"] / 1e9, 3)}
    out["total_ms"] = round(sum(v["ms"] for v in out.values()), 3)
    return out


def model_case(depth, V, B, hw, steps, warmup):
    m = MultiViewGaze(depth, 3)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.make_state_dict(depth, 0, 3).items()})
    m.to(dev)
    m.ensure_layout()
    assert not m._backbone.split
    inp = synth.make_inputs(B, V, 1234, hw)
    img = [torch.from_numpy(inp["img"][:, v]).contiguous().to(dev) for v in range(V)]
    rot = rotation_matrix_2d(torch.from_numpy(inp["head_pose"]).reshape(-1, 2).to(dev)).reshape(B, V, 3, 3).contiguous()
    gt = torch.from_numpy(inp["gt_gaze"]).to(dev)
    crit = MultiViewIterationLoss(rel_weight=0.01, reference_decay=1.0, iter_decay=0.5)

    def step():
        m.zero_grad(set_to_none=False)
        crit(m.forward_multiview(img, rot), gt).backward()
    res = {}
    for mode in ("train", "eval"):
        m.train(mode == "train")
        med, best = event_ms(step, steps, warmup)
        res[mode] = {"step_ms_median": round(med, 3), "step_ms_min": round(best, 3), "bn_backward": bn_family(step)}
    res["eval_over_train_step"] = round(res["eval"]["step_ms_median"] / res["train"]["step_ms_median"], 3)
    res["eval_over_train_bn_backward"] = round(res["eval"]["bn_backward"]["total_ms"] / res["train"]["bn_backward"]["total_ms"], 3)
    return res


def pass_rates(N=32, G=4, iters=10):
    """Per ResNet-50 stage shape: the train pair (reduce with the mask + apply) vs the eval one-pass kernel, TB/s on the
    algorithmic bytes (fp32: 12 B per element for a pass that reads g, y and writes dy; + 1/16 for mask bits)."""
    rows_out = []
    for hw, C, res in [(56, 64, False), (56, 256, True), (28, 128, False), (28, 512, True), (14, 256, False), (14, 1024, True),
                       (7, 512, False), (7, 2048, True)]:
        rows = N * hw * hw
        n = G * rows * C
        y, g = torch.randn(G, rows, C, device=dev), torch.randn(G, rows, C, device=dev)
        scale, shift = torch.rand(G, C, device=dev) + 0.5, torch.randn(G, C, device=dev) * 0.3
        mean, invstd = torch.randn(G, C, device=dev) * 0.1, torch.rand(G, C, device=dev) + 0.5
        gamma, rm, rv = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.1, torch.rand(C, device=dev) + 0.5
        s1, s2 = torch.empty(G, C, device=dev), torch.empty(G, C, device=dev)
        dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
        dy = torch.empty_like(g)
        bits = torch.randint(0, 255, (n // 4,), dtype=torch.uint8, device=dev) if res else None
        mask = {"relu_bits": bits} if res else {"relu_affine": (scale, shift)}

        def train_pair():
            if res:
                ops.bn_bwd_reduce_bits(g, bits, y, mean, invstd, G, rows, C, s1, s2, dg, db, False, dz_out=g)
                ops.bn_bwd_apply(g, None, y, mean, invstd, gamma, s1, s2, G, rows, C, dy)
            else:
                ops.bn_bwd_reduce(g, None, y, mean, invstd, G, rows, C, s1, s2, dg, db, False, (scale, shift))
                ops.bn_bwd_apply(g, None, y, mean, invstd, gamma, s1, s2, G, rows, C, dy, None, (scale, shift))

        def eval_pass():
            ops.bn_eval_bwd(g, y, gamma, rm, rv, 1e-5, G, rows, C, dy, dg, db, False, dz_out=g if res else None, **mask)
        t_tr, _ = event_ms(train_pair, iters, 2)
        t_ev, _ = event_ms(eval_pass, iters, 2)
        b_ev = n * (12 + (4 if res else 0) + (0.25 if res else 0))            # g, y in; dy (+ dz) out (+ bits)
        b_tr = n * ((12.25 if res else 8) + 12)                                # reduce (+ dz store) + apply
        rows_out.append({"shape": f"{G}x{rows}x{C}" + (" residual" if res else ""), "train_pair_ms": round(t_tr, 4),
                         "eval_ms": round(t_ev, 4), "eval_over_train": round(t_ev / t_tr, 3),
                         "train_pair_TBps": round(b_tr / t_tr / 1e9, 2), "eval_TBps": round(b_ev / t_ev / 1e9, 2)})
        del y, g, dy
    return rows_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "conv_family": "fp32-MFMA (MVG_SPLIT=0) in both modes", "cases": {}}
    for name, depth, V, B, hw in CASES:
        out["cases"][name] = model_case(depth, V, B, hw, a.steps, a.warmup)
        print(name, json.dumps(out["cases"][name]), flush=True)
        torch.cuda.empty_cache()
    out["bn_backward_passes_r50_n32_g4"] = pass_rates()
    for r in out["bn_backward_passes_r50_n32_g4"]:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
