#!/usr/bin/env python3
"""Frozen-BatchNorm training steps (model.train() with model.freeze_batchnorm: BatchNorm on its running statistics, the one-pass
backward of bn.hip) on the bf16 path against the bf16 train-mode step, and the fp32 eval-mode step at the same shapes; the
event-timed BatchNorm-backward family of each (the one-pass kernel is counted under bn_bwd_apply) and the streaming rate of the
bf16 BatchNorm-backward passes per ResNet-50 shape.  Synthetic weights and inputs; the sibling of eval_step_bench.py, whose
timing helpers it uses (that module sets MVG_SPLIT=0, which neither the bf16 path nor an eval-mode tape reads).
Usage: frozen_step_bench.py [--steps K] [--warmup W] [--out FILE.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from eval_step_bench import CASES, bn_family, dev, event_ms  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rot_mvgaze_amd import ops, synth  # noqa: E402
from rot_mvgaze_amd.geometry import rotation_matrix_2d  # noqa: E402
from rot_mvgaze_amd.losses import MultiViewIterationLoss  # noqa: E402
from rot_mvgaze_amd.model import MultiViewGaze  # noqa: E402


def model_case(depth, V, B, hw, steps, warmup):
    m = MultiViewGaze(depth, 3)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.make_state_dict(depth, 0, 3).items()})
    m.to(dev)
    inp = synth.make_inputs(B, V, 1234, hw)
    img = [torch.from_numpy(inp["img"][:, v]).contiguous().to(dev) for v in range(V)]
    rot = rotation_matrix_2d(torch.from_numpy(inp["head_pose"]).reshape(-1, 2).to(dev)).reshape(B, V, 3, 3).contiguous()
    gt = torch.from_numpy(inp["gt_gaze"]).to(dev)
    crit = MultiViewIterationLoss(rel_weight=0.01, reference_decay=1.0, iter_decay=0.5)

    def step():
        m.zero_grad(set_to_none=False)
        crit(m.forward_multiview(img, rot), gt).backward()
    res = {}
    # (frozen steps first: the train-mode steps move the running statistics)
    for mode, dtype, train, frozen in (("bf16_frozen", torch.bfloat16, True, True), ("fp32_eval", torch.float32, False, False),
                                       ("bf16_train", torch.bfloat16, True, False)):
        m.compute_dtype, m.freeze_batchnorm = dtype, frozen
        m.train(train)
        med, best = event_ms(step, steps, warmup)
        res[mode] = {"step_ms_median": round(med, 3), "step_ms_min": round(best, 3), "bn_backward": bn_family(step)}
    res["bf16_frozen_over_train_step"] = round(res["bf16_frozen"]["step_ms_median"] / res["bf16_train"]["step_ms_median"], 3)
    res["bf16_frozen_over_train_bn_backward"] = round(res["bf16_frozen"]["bn_backward"]["total_ms"] / res["bf16_train"]["bn_backward"]["total_ms"], 3)
    return res


def pass_rates(N=32, G=4, iters=10):
    """Per ResNet-50 stage shape, bf16 storage: the train pair (reduce with the mask + apply) against the one-pass kernel, TB/s on
    the algorithmic bytes (2 B per element read or written: 6 B for a pass that reads g, y and writes dy; + 1/8 for mask bits)."""
    rows_out = []
    for hw, C, res in [(56, 64, False), (56, 256, True), (28, 128, False), (28, 512, True), (14, 256, False), (14, 1024, True),
                       (7, 512, False), (7, 2048, True)]:
        rows = N * hw * hw
        n = G * rows * C
        y, g = (torch.randn(G, rows, C, device=dev).to(torch.bfloat16) for _ in range(2))
        scale, shift = torch.rand(G, C, device=dev) + 0.5, torch.randn(G, C, device=dev) * 0.3
        mean, invstd = torch.randn(G, C, device=dev) * 0.1, torch.rand(G, C, device=dev) + 0.5
        gamma, rm, rv = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.1, torch.rand(C, device=dev) + 0.5
        s1, s2 = torch.empty(G, C, device=dev), torch.empty(G, C, device=dev)
        dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
        dy = torch.empty_like(g)
        bits = torch.randint(0, 255, (n // 8,), dtype=torch.uint8, device=dev) if res else None
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
        b_ev = n * (6 + (2 if res else 0) + (0.125 if res else 0))             # g, y in; dy (+ dz) out (+ bits)
        b_tr = n * ((6.125 if res else 4) + 6)                                  # reduce (+ dz store) + apply
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
    out = {"device": torch.cuda.get_device_name(0), "cases": {}}
    for name, depth, V, B, hw in CASES:
        out["cases"][name] = model_case(depth, V, B, hw, a.steps, a.warmup)
        print(name, json.dumps(out["cases"][name]), flush=True)
        torch.cuda.empty_cache()
    out["bf16_bn_backward_passes_r50_n32_g4"] = pass_rates()
    for r in out["bf16_bn_backward_passes_r50_n32_g4"]:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
