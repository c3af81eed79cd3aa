#!/usr/bin/env python3
"""mvg_augment_u8hwc against Pillow itself (ImageEnhance.{Brightness, Contrast, Color} in a random order, then
Image.transform(AFFINE, NEAREST)) for random image sizes, factors, scales and translations, batches of mixed records:
augment_fuzz.py [cases] [seed]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from PIL import Image, ImageEnhance
import rot_mvgaze_amd
from rot_mvgaze_amd.augment import REC_DTYPE, AugmentDraws, TrainAugment, inverse_affine
cases = int(sys.argv[1]) if len(sys.argv) > 1 else 40
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
dev = torch.device("cuda:0")
aug = TrainAugment()
ENH = [ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color]
bad = 0
for it in range(cases):
    B = int(rng.integers(1, 6))
    H, W = (int(rng.integers(1, 300)), int(rng.integers(1, 300))) if it % 4 else (224, 224)
    bgr = bool(rng.integers(0, 2))
    lo, hi = sorted(int(v) for v in rng.integers(0, 257, 2))
    img = rng.integers(lo, max(hi, lo + 1), (B, H, W, 3), dtype=np.uint8)
    recs = np.zeros(B, dtype=REC_DTYPE)
    ref = np.empty_like(img)
    for b in range(B):
        recs["order"][b] = rng.permutation(3)
        recs["factor"][b] = [rng.choice([0.0, 1.0, 2.0, 2.0 * rng.random()]) for _ in range(3)]
        m = inverse_affine(H, W, 0.8 + 0.45 * rng.random(), int(rng.integers(-W // 5 - 1, W // 5 + 2)), int(rng.integers(-H // 5 - 1, H // 5 + 2)))
        recs["a0"][b], recs["cx"][b], recs["a4"][b], recs["cy"][b] = m
        pil = Image.fromarray(np.ascontiguousarray(img[b, ..., ::-1] if bgr else img[b]), "RGB")
        for op in recs["order"][b]:
            pil = ENH[int(op)](pil).enhance(float(recs["factor"][b][int(op)]))
        ref[b] = np.asarray(pil.transform((W, H), Image.AFFINE, [m[0], 0.0, m[1], 0.0, m[2], m[3]], Image.NEAREST))
    got = aug.apply(torch.from_numpy(img).to(dev), AugmentDraws(recs, None), out="u8", bgr=bgr).cpu().numpy()
    ok = np.array_equal(got, ref)
    bad += not ok
    print(("ok  " if ok else "FAIL"), f"B{B} {H}x{W} bgr={int(bgr)} range [{lo}, {hi})", "" if ok else f"mismatches {(got != ref).sum()}", flush=True)
print("failures:", bad)
sys.exit(1 if bad else 0)
