#!/usr/bin/env python3
"""One view's input of a bf16 training step from raw uint8 patches, two forms on the same batch and draws, on one box:
the single launch into the stem's row windows (mvg_augment_u8hwc_bf16) against the chain it replaces - augment -> fp32
NHWC4 (mvg_augment_u8hwc), nhwc4_to_nchw, stem_rowwindow_bf16 - timed as the three launches back to back (their sum) and
each alone.  Both with the erase at p = 0.5.  hipEvents around 20 calls after a warm-up, the two forms alternated over 5
rounds; median and spread (max - min over the rounds) reported.  Cases: 64 images of 224 x 224 (C5's per-view batch) and 512.

    python scripts/augment_bf16_bench.py [--out profiles/r16_augment_bf16_bench.json]
"""
import argparse, json, os, random, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import rot_mvgaze_amd
from rot_mvgaze_amd import ops
from rot_mvgaze_amd.augment import RandomMultiErasing, TrainAugment
from rot_mvgaze_amd.backbone import IMAGE_MEAN, IMAGE_STD

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_augment_bf16_bench.json"))
args = ap.parse_args()
dev = torch.device("cuda:0")
H = W = 224
ITERS, ROUNDS = 20, 5


def events_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ITERS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / ITERS


result = {"device": torch.cuda.get_device_name(0), "h": H, "w": W, "iters": ITERS, "rounds": ROUNDS, "erase_p": 0.5,
          "bytes_per_image": {"single": H * W * (6 + 32), "chain": H * W * (6 + 16 + 16 + 12 + 12 + 32)}, "cases": []}
for n in (64, 512):
    torch.manual_seed(0), random.seed(0), np.random.seed(0)
    u8 = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device=dev)
    aug = TrainAugment(erase=RandomMultiErasing(p=0.5, proportion=[0.5, 0.6], dot_size=[0.05, 0.3]))
    draws = aug.draw(n, H, W)
    recs = torch.from_numpy(draws.recs.view(np.uint8).reshape(-1)).to(dev)
    gmax = max(g for g, _ in draws.erase)
    mh, gh = torch.zeros(n, gmax * gmax, dtype=torch.float32), torch.zeros(n, dtype=torch.int32)
    for i, (g, m) in enumerate(draws.erase):
        gh[i] = g
        if g:
            mh[i, : g * g] = m.reshape(-1)
    masks, grid = mh.to(dev), gh.to(dev)
    nhwc4 = torch.empty(n, H, W, 4, dtype=torch.float32, device=dev)
    nchw = torch.empty(n, 3, H, W, dtype=torch.float32, device=dev)
    rw_chain = torch.empty(n, H, W // 4, 64, dtype=torch.bfloat16, device=dev)
    rw_single = torch.empty(n, H, W // 4, 64, dtype=torch.bfloat16, device=dev)

    def single():
        ops.augment_u8hwc_bf16(u8, recs, None, rw_single, masks, grid, gmax, n, H, W, IMAGE_MEAN, IMAGE_STD, True)

    def chain_augment():
        ops.augment_u8hwc(u8, recs, None, nhwc4, masks, grid, gmax, n, H, W, IMAGE_MEAN, IMAGE_STD, True)

    def chain_nchw():
        ops.nhwc4_to_nchw(nhwc4, nchw, n, 3, H, W)

    def chain_windows():
        ops.stem_rowwindow_bf16(nchw, rw_chain)

    def chain():
        chain_augment(), chain_nchw(), chain_windows()
    for fn in (single, chain):                           # warm-up: code objects, clocks
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    assert torch.equal(rw_single.view(torch.int16), rw_chain.view(torch.int16))           # the two forms agree bit for bit
    t_single, t_chain = [], []
    for _ in range(ROUNDS):
        t_single.append(events_ms(single))
        t_chain.append(events_ms(chain))
    parts = {name: statistics.median(events_ms(fn) for _ in range(ROUNDS))
             for name, fn in (("augment_u8hwc_ms", chain_augment), ("nhwc4_to_nchw_ms", chain_nchw), ("stem_rowwindow_bf16_ms", chain_windows))}
    s, c = statistics.median(t_single), statistics.median(t_chain)
    case = {"n": n, "single_ms": s, "chain_ms": c, "ratio": s / c, "single_spread_ms": max(t_single) - min(t_single),
            "chain_spread_ms": max(t_chain) - min(t_chain), "single_ms_rounds": t_single, "chain_ms_rounds": t_chain,
            "chain_parts_alone": parts, "single_GBps": n * H * W * 38.0 / s / 1e6, "chain_GBps": n * H * W * 94.0 / c / 1e6}
    result["cases"].append(case)
    print(f"n={n:4d}: single launch {s:.4f} ms (spread {case['single_spread_ms']:.4f})   chain {c:.4f} ms (spread "
          f"{case['chain_spread_ms']:.4f})   ratio {s / c:.2f}   parts alone {parts}")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
print(args.out)
