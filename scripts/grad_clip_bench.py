#!/usr/bin/env python3
"""The optimizer step alone, with and without global-norm gradient clipping, on the ResNet-50 model's arena (the parameter count
of BASELINE config C3; the gradients come from one real backward at a small batch - the step's cost depends on the arena only):
  a_unclipped    optim.Adam.step() of the plan as it is without clipping (the parent's code path: also the check that it did not move)
  b_clipped      optim.Adam(max_grad_norm=...).step(): mvg_grad_norm_segments, then the clipped segmented update
  c_torch_clip   torch.nn.utils.clip_grad_norm_ over the trainable parameters (arena views), then a_unclipped
in three modes:
  whole          one group, nothing frozen, capturable=False (a = the one-launch mvg_adam_step)
  frozen_stem    head and backbone groups, the stem and layer1 frozen, capturable=False (a = mvg_adam_step_segments)
  captured       frozen_stem with capturable="segments", each form's step captured in a hipGraph and replayed (b with the guard on)
Device events around CALLS back-to-back steps, ROUNDS rounds that alternate the three forms, the gradient arena restored in front
of every timed window (c rewrites it); median over rounds and the round-to-round spread; the host's own time per step next to it.
b - a is held against the time a 4 B / element read takes at the rate a itself achieves on its 28 B / element (a / 7).
Usage: grad_clip_bench.py [--calls 20] [--rounds 5] [--out FILE.json]"""
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
from rot_mvgaze_amd.losses import MultiViewIterationLoss  # noqa: E402
from rot_mvgaze_amd.model import MultiViewGaze  # noqa: E402
from rot_mvgaze_amd.optim import Adam  # noqa: E402

dev = torch.device("cuda:0")
BB = "_feat_extractor.0."


def frozen_name(name):
    """The stem and layer1."""
    return name.startswith(BB) and ".fc." not in name and not any(f".layer{i}." in name for i in (2, 3, 4))


def model_with_gradients(freeze: bool):
    m = MultiViewGaze(50, 3).to(dev).train()
    if freeze:
        for k, p in m.named_parameters():
            if frozen_name(k):
                p.requires_grad_(False)
    B, V, hw = 2, 2, 64
    inp = synth.make_inputs(B, V, 77, hw)
    img = [torch.from_numpy(np.ascontiguousarray(inp["img"][:, v])).to(dev) for v in range(V)]
    gt = torch.from_numpy(inp["gt_gaze"]).to(dev)
    rot = rotation_matrix_2d(torch.from_numpy(inp["head_pose"]).reshape(-1, 2).to(dev)).reshape(B, V, 3, 3)
    crit = MultiViewIterationLoss(rel_weight=0.01, reference_decay=1.0, iter_decay=0.5)
    crit(m.forward_multiview(img, rot), gt).backward()
    torch.cuda.synchronize()
    return m


def groups_of(m, two: bool):
    if not two:
        return [p for p in m.parameters()]
    head = [p for k, p in m.named_parameters() if not k.startswith("_feat_extractor")]
    bb = [p for k, p in m.named_parameters() if k.startswith("_feat_extractor") and p.requires_grad]
    return [{"params": head, "lr": 1e-3, "weight_decay": 0.0}, {"params": bb, "lr": 1e-4, "weight_decay": 1e-6}]


def measure(runs, restore, calls, rounds):
    for fn in runs.values():                              # every form once: code objects loaded, optimizer state created
        restore()
        fn()
    torch.cuda.synchronize()
    gpu, host = {k: [] for k in runs}, {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            restore()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            h0 = time.perf_counter()
            t0.record()
            for _ in range(calls):
                fn()
            t1.record()
            host[k].append((time.perf_counter() - h0) * 1e3 / calls)
            t1.synchronize()
            gpu[k].append(t0.elapsed_time(t1) / calls)
    return {k: {"ms_per_step_median": round(float(np.median(gpu[k])), 4), "ms_per_step_min": round(min(gpu[k]), 4),
                "ms_per_step_max": round(max(gpu[k]), 4), "host_ms_per_step_median": round(float(np.median(host[k])), 4)} for k in runs}


def mode(m, two_groups: bool, captured: bool, calls: int, rounds: int):
    arena_g, entries = m.grad_arena()
    trainable = [p for (p, _, _) in entries if p.grad is not None]
    active = sum((n + 3) // 4 * 4 for (p, _, n) in entries if p.grad is not None)
    saved = arena_g.clone()
    norm = float(torch.linalg.vector_norm(saved.double()).item())          # (frozen ranges of the arena hold zeros)
    max_norm = 0.5 * norm                                                  # the clip binds
    cap = "segments" if captured else False
    plain = Adam(groups_of(m, two_groups), lr=1e-4, weight_decay=1e-6, capturable=cap)
    plain_c = Adam(groups_of(m, two_groups), lr=1e-4, weight_decay=1e-6, capturable=cap)
    clipped = Adam(groups_of(m, two_groups), lr=1e-4, weight_decay=1e-6, capturable=cap, max_grad_norm=max_norm, skip_nonfinite=captured)

    def torch_clip():
        torch.nn.utils.clip_grad_norm_(trainable, max_norm)
        plain_c.step()
    runs = {"a_unclipped": plain.step, "b_clipped": clipped.step, "c_torch_clip": torch_clip}
    notes = {}
    if captured:
        for fn in runs.values():                          # the eager step that creates the device state, then the capture
            arena_g.copy_(saved)
            fn()
        torch.cuda.synchronize()
        graphs = {}
        for k, fn in runs.items():
            arena_g.copy_(saved)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(g):
                    fn()
                graphs[k] = g.replay
            except Exception as e:                        # (a form that cannot be captured is timed eagerly, and said so)
                torch.cuda.synchronize()
                notes[k] = f"not capturable, timed eagerly: {type(e).__name__}: {str(e)[:200]}"
                graphs[k] = fn
        runs = graphs
    out = measure(runs, lambda: arena_g.copy_(saved), calls, rounds)
    arena_g.copy_(saved)                                  # (the next mode starts from the gradient this one found)
    rep = clipped.grad_clip_report()[0]
    a, b, c = (out[k]["ms_per_step_median"] for k in ("a_unclipped", "b_clipped", "c_torch_clip"))
    read_ms = a / 7.0                                     # 4 B per element at the rate a moves its 28 B per element
    out["summary"] = {"active_elements": active, "trainable_tensors": len(trainable), "grad_norm": norm, "max_grad_norm": max_norm,
                      "recorded": rep, "a_GBps_on_28B": round(28.0 * active / a / 1e6, 1), "b_over_a": round(b / a, 4),
                      "c_over_a": round(c / a, 4), "b_minus_a_ms": round(b - a, 4), "read_4B_at_a_rate_ms": round(read_ms, 4),
                      "b_minus_a_over_read": round((b - a) / read_ms, 3), "b_below_c": bool(b < c)}
    if notes:
        out["notes"] = notes
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "calls_per_round": a.calls, "rounds": a.rounds, "modes": {}}
    m = model_with_gradients(freeze=False)
    out["arena_elements"] = m.param_arena().numel()
    out["modes"]["whole"] = mode(m, False, False, a.calls, a.rounds)
    print("whole", json.dumps(out["modes"]["whole"]), flush=True)
    del m
    torch.cuda.empty_cache()
    m = model_with_gradients(freeze=True)
    for name, captured in (("frozen_stem", False), ("captured", True)):
        out["modes"][name] = mode(m, True, captured, a.calls, a.rounds)
        print(name, json.dumps(out["modes"][name]), flush=True)
    out["b_below_c_in_every_mode"] = all(v["summary"]["b_below_c"] for v in out["modes"].values())
    print(json.dumps({"b_below_c_in_every_mode": out["b_below_c_in_every_mode"]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
