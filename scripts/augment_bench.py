#!/usr/bin/env python3
"""The augmenting raw-input launch (mvg_augment_u8hwc: ColorJitter + RandomAffine + ToTensor + Normalize) against
mvg_preprocess_u8hwc alone - the un-augmented raw path - on the same uint8 batch, on one box: hipEvents around 20 calls
after a warm-up, the two alternated over 5 rounds (median reported).  Cases: the C3 input, 512 images of 224 x 224, and
16 images.  Also the host side of a step: TrainAugment.draw and the whole apply (records copy included), wall clock.

    python scripts/augment_bench.py [--out profiles/r13_augment_bench.json]
"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import rot_mvgaze_amd
from rot_mvgaze_amd import ops
from rot_mvgaze_amd.augment import RandomMultiErasing, TrainAugment
from rot_mvgaze_amd.backbone import IMAGE_MEAN, IMAGE_STD

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_augment_bench.json"))
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


def wall_ms(fn, iters=5):
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


result = {"device": torch.cuda.get_device_name(0), "h": H, "w": W, "iters": ITERS, "rounds": ROUNDS, "cases": []}
for n in (512, 16):
    torch.manual_seed(0)
    u8 = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device=dev)
    dst = torch.empty(n, H, W, 4, dtype=torch.float32, device=dev)
    aug = TrainAugment()
    draws = aug.draw(n, H, W)
    recs = torch.from_numpy(draws.recs.view(np.uint8).reshape(-1)).to(dev)
    erase = TrainAugment(erase=RandomMultiErasing(p=0.5, proportion=[0.5, 0.6], dot_size=[0.05, 0.3]))

    def plain():
        ops.preprocess_u8hwc(u8, dst, n, H, W, IMAGE_MEAN, IMAGE_STD, True)

    def augment():
        ops.augment_u8hwc(u8, recs, None, dst, None, None, 0, n, H, W, IMAGE_MEAN, IMAGE_STD, True)
    for fn in (plain, augment):                          # warm-up: code objects, clocks
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t_plain, t_aug = [], []
    for _ in range(ROUNDS):
        t_plain.append(events_ms(plain))
        t_aug.append(events_ms(augment))
    p, a = statistics.median(t_plain), statistics.median(t_aug)
    px = n * H * W
    case = {"n": n, "preprocess_u8hwc_ms": p, "augment_u8hwc_ms": a, "ratio": a / p,
            "preprocess_u8hwc_ms_rounds": t_plain, "augment_u8hwc_ms_rounds": t_aug,
            "augment_GBps": px * 22.0 / a / 1e6, "preprocess_GBps": px * 19.0 / p / 1e6,
            "draw_host_ms": wall_ms(lambda: aug.draw(n, H, W)),
            "draw_with_erase_host_ms": wall_ms(lambda: erase.draw(n, H, W)),
            "apply_wall_ms": wall_ms(lambda: aug.apply(u8, draws, out="nhwc4", bgr=True))}
    result["cases"].append(case)
    print(f"n={n:4d}: preprocess_u8hwc {p:.4f} ms   augment_u8hwc {a:.4f} ms   ratio {a / p:.2f}   "
          f"draw (host) {case['draw_host_ms']:.2f} ms   apply incl. record copy {case['apply_wall_ms']:.3f} ms")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
print(args.out)
