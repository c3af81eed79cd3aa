#!/usr/bin/env python3
"""What TrainAugment(draws="device") costs and buys, at BASELINE config C3's shapes (B = 128 per view, V = 4, 224 x 224 BGR
uint8 patches, the reference recipe with the erase on), three parts in ONE process:
  draws     host ms per step (V views) of the draws plus what carries them to the device - the launch into the fp32 stem
            operand included - in host mode (TrainAugment.draw + launch: the host loop and three copies per view) and in device
            mode (draw_device + launch: two ctypes calls per view); the draw call alone in both modes.  `host` stops when the
            last launch is queued, `wall` after the device synchronise that follows.  ROUNDS rounds alternate the two modes.
  kernels   device time of one draw launch next to one pixel launch (mvg_augment_draw | mvg_augment_u8hwc into NHWC4, B = 128):
            the library's per-launch event brackets (ops.prof_*), LAUNCHES launches each, so a launch's event overhead is in both.
  captured  ResNet-50, V = 4, B = 32, raw uint8 static inputs: host ms per replay of graph.GraphedStep over a device-draw
            input_augment and optim.Adam(capturable=True), next to the eager step with device draws and with host draws
            (host / wall / device-event ms per step; rounds alternate the three).
No figure is gated.  Synthetic weights and inputs.
Usage: augment_draw_bench.py [--batch 128] [--views 4] [--hw 224] [--steps 10] [--rounds 5] [--launches 50] [--model-batch 32]
                             [--skip-model] [--out FILE.json]"""
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
from rot_mvgaze_amd import ops, synth  # noqa: E402
from rot_mvgaze_amd.augment import RandomMultiErasing, TrainAugment  # noqa: E402

dev = torch.device("cuda:0")


def recipe(draws):
    return TrainAugment(erase=RandomMultiErasing([0.5, 0.6], 0.5, [0.05, 0.3]), draws=draws, seed=1234 if draws == "device" else None)


def stats(ts):
    return {"median": round(float(np.median(ts)), 4), "min": round(float(min(ts)), 4), "max": round(float(max(ts)), 4)}


def clocked(fn, steps):
    """(host, wall) ms per call of fn: host until the last call returned, wall after the synchronise that follows."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3 / steps, (t2 - t0) * 1e3 / steps


def part_draws(a):
    B, V, hw = a.batch, a.views, a.hw
    rng = np.random.RandomState(1)
    u8 = [torch.from_numpy(rng.randint(0, 256, (B, hw, hw, 3)).astype(np.uint8)).to(dev) for _ in range(V)]
    x0 = torch.empty(V, B, hw, hw, 4, dtype=torch.float32, device=dev)
    augs = {"host": recipe("host"), "device": recipe("device")}

    def draw_of(mode):
        aug = augs[mode]
        return (lambda: aug.draw_device(B, hw, hw, dev)) if mode == "device" else (lambda: aug.draw(B, hw, hw))

    def step_of(mode):
        aug, draw = augs[mode], draw_of(mode)

        def step():
            for v in range(V):
                aug.launch(u8[v], draw(), None, x0[v], True)
        return step

    def draws_only_of(mode):
        draw = draw_of(mode)

        def step():
            for v in range(V):
                draw()
        return step
    ms = {mode: {"draw_and_launch_host": [], "draw_and_launch_wall": [], "draw_only_host": []} for mode in augs}
    for mode in augs:
        step_of(mode)()                                   # warm-up: code objects, the launch counter, allocator pools
    for _ in range(a.rounds):
        for mode in augs:
            host, wall = clocked(step_of(mode), a.steps)
            ms[mode]["draw_and_launch_host"].append(host)
            ms[mode]["draw_and_launch_wall"].append(wall)
            ms[mode]["draw_only_host"].append(clocked(draws_only_of(mode), a.steps)[0])
    res = {mode: {k + "_ms_per_step": stats(ts) for k, ts in d.items()} for mode, d in ms.items()}
    res["torch_calls_note"] = "a step is V views; host mode draws image by image on the host and copies records, masks and grid per view"
    for mode in augs:
        print("draws", mode, json.dumps(res[mode]), flush=True)

    # ---- kernels: one draw launch next to one pixel launch, event-bracketed by the library
    aug = augs["device"]
    d = aug.draw_device(B, hw, hw, dev)
    torch.cuda.synchronize()
    kern = {}
    for name, fn in (("draw_launch", lambda: aug.draw_device(B, hw, hw, dev)), ("pixel_launch_nhwc4", lambda: aug.launch(u8[0], d, None, x0[0], True))):
        fn()
        torch.cuda.synchronize()
        ops.prof_enable(True)
        ops.prof_reset()
        for _ in range(a.launches):
            fn()
        torch.cuda.synchronize()
        got = ops.prof_collect()
        ops.prof_enable(False)
        (fam, e), = got.items()
        assert e["launches"] == a.launches, got
        kern[name] = {"family": fam, "launches": e["launches"], "device_us_per_launch": round(e["ms"] * 1e3 / e["launches"], 2)}
        print("kernels", name, json.dumps(kern[name]), flush=True)
    return res, kern


def part_captured(a):
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    from rot_mvgaze_amd.graph import GraphedStep
    from rot_mvgaze_amd.losses import MultiViewIterationLoss
    from rot_mvgaze_amd.model import MultiViewGaze
    from rot_mvgaze_amd.optim import Adam
    V, B, hw = a.views, a.model_batch, a.hw
    weights = {k: torch.from_numpy(np.array(v)) for k, v in synth.make_state_dict(50, 0, 3).items()}
    rng = np.random.RandomState(2)
    img = [torch.from_numpy(rng.randint(0, 256, (B, hw, hw, 3)).astype(np.uint8)).to(dev) for _ in range(V)]
    inp = synth.make_inputs(B, V, 1234, 8)                # (poses and labels only: the patches above are the input)
    gt = torch.from_numpy(inp["gt_gaze"]).to(dev)
    rot = rotation_matrix_2d(torch.from_numpy(inp["head_pose"]).reshape(-1, 2).to(dev)).reshape(B, V, 3, 3)

    def build(draws, capturable):
        m = MultiViewGaze(50, 3)
        m.load_state_dict(weights, strict=True)
        m.to(dev).train()
        m.input_augment, m.input_bgr, m.input_size = recipe(draws), True, None
        opt = Adam(m.parameters(), lr=1e-4, weight_decay=1e-6, capturable=capturable)
        crit = MultiViewIterationLoss(rel_weight=0.01, reference_decay=1.0, iter_decay=0.5)

        def step():
            m.zero_grad(set_to_none=True)
            loss = crit(m.forward_multiview(img, rot), gt)
            loss.backward()
            opt.step()
            return loss
        return m, opt, step
    arms = {}
    for name, draws in (("eager_host_draws", "host"), ("eager_device_draws", "device")):
        _, _, step = build(draws, False)
        for _ in range(2):
            step()
        arms[name] = step
    mg, og, graphed = build("device", True)
    gs = GraphedStep(mg, graphed, og, warmup=3)
    gs.run()
    arms["captured_device_draws"] = gs.run
    torch.cuda.synchronize()
    ms = {name: {"host": [], "wall": [], "device": []} for name in arms}
    for _ in range(a.rounds):
        for name, fn in arms.items():
            fn()                                          # (the first step after a switch: not timed)
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
    res = {name: {what + "_ms_per_step": stats(ts) for what, ts in d.items()} for name, d in ms.items()}
    for name in res:
        print("captured", name, json.dumps(res[name]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--model-batch", type=int, default=32)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_draw_bench.py measures on the GPU: no device found")
    out = {"device": torch.cuda.get_device_name(0), "views": a.views, "batch_per_view": a.batch, "input": f"{a.hw}x{a.hw}x3 uint8 BGR",
           "recipe": "brightness 1.0, contrast 0.1, saturation 0.1, scale [0.99, 1.01], translate 0.01, erase p 0.5 proportion [0.5, 0.6] dot [0.05, 0.3]",
           "steps_per_round": a.steps, "rounds": a.rounds}
    out["draws"], out["kernels"] = part_draws(a)
    if not a.skip_model:
        out["captured_step"] = dict(part_captured(a), model="ResNet-50", batch=a.model_batch, views=a.views)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f_:
            json.dump(out, f_, indent=1)


if __name__ == "__main__":
    main()
