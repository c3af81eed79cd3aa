#!/usr/bin/env python3
"""Writes tests/golden/color_affine.npz: small uint8 images put through Pillow's ImageEnhance.{Brightness, Contrast,
Color} in a per-image order and Image.transform(AFFINE, NEAREST) - the calls torchvision's ColorJitter and RandomAffine
make on a PIL image (the reference's training transform, main.py:41-49) - with the per-image parameters.  Needs Pillow
(the fixture was written with the version printed at the end); the tests read only the .npz.

Before writing, the NumPy restatement (tests/augment_ref.py) is held against Pillow on every case and on random
224 x 224 images, so a fixture is only written from a restatement that agrees.

    in_XX  uint8 [h, w, 3]  source image in its stored channel order (swap[XX] = 1: BGR)
    out_XX uint8 [h, w, 3]  Pillow's result (RGB)
    factors float64 [n, 3]  brightness, contrast, saturation factor
    order   int32   [n, 3]  op ids in the order applied (0 brightness, 1 contrast, 2 saturation)
    matrix  float64 [n, 4]  a0, c_x, a4, c_y of the inverse affine map
    swap    int32   [n]
"""
import itertools
import os
import sys

import numpy as np
import PIL
from PIL import Image, ImageEnhance

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import augment_ref as R  # noqa: E402

ENHANCERS = {R.BRIGHTNESS: ImageEnhance.Brightness, R.CONTRAST: ImageEnhance.Contrast, R.SATURATION: ImageEnhance.Color}


def pillow(u8, factors, order, matrix, swap):
    img = Image.fromarray(np.ascontiguousarray(u8[..., ::-1] if swap else u8), "RGB")
    for op in order:
        img = ENHANCERS[int(op)](img).enhance(float(factors[int(op)]))
    h, w = u8.shape[:2]
    a0, cx, a4, cy = (float(m) for m in matrix)
    img = img.transform((w, h), Image.AFFINE, [a0, 0.0, cx, 0.0, a4, cy], Image.NEAREST)
    return np.asarray(img)


def cases():
    rng = np.random.RandomState(20240613)
    orders = list(itertools.permutations((0, 1, 2)))
    out = []

    def add(img, factors, order, scale, tx, ty, swap):
        h, w = img.shape[:2]
        out.append((img.astype(np.uint8), np.array(factors, np.float64), np.array(order, np.int32),
                    np.array(R.affine_matrix(h, w, scale, tx, ty), np.float64), int(swap)))

    sizes = [(40, 56), (17, 23), (33, 31), (8, 8), (39, 55), (5, 3)]
    # all six orders, twice: factors near the recipe's, then wide ones; scale below / above 1, fill on every side
    shifts = [(0, 0), (3, 0), (-3, 0), (0, 4), (0, -4), (2, -2)]
    for k, order in enumerate(orders):
        h, w = sizes[k]
        add(rng.randint(0, 256, (h, w, 3)), (0.9 + 0.2 * rng.rand(), 0.9 + 0.2 * rng.rand(), 0.9 + 0.2 * rng.rand()), order,
            0.99 + 0.02 * rng.rand(), *shifts[k], k % 2)
    for k, order in enumerate(orders):
        h, w = sizes[(k + 2) % 6]
        add(rng.randint(0, 256, (h, w, 3)), (2.0 * rng.rand(), 2.0 * rng.rand(), 2.0 * rng.rand()), order,
            (0.8, 1.25, 0.93, 1.1, 1.0, 0.99)[k], *shifts[5 - k], (k + 1) % 2)
    # factors at the end points and at 0.9 / 1.1, one op at a time and together
    for k, f in enumerate((0.0, 1.0, 2.0, 0.9, 1.1)):
        for op in range(3):
            fs = [1.0, 1.0, 1.0]
            fs[op] = f
            h, w = sizes[(k + op) % 6]
            add(rng.randint(0, 256, (h, w, 3)), fs, orders[(k + op) % 6], (1.0, 1.01, 0.99)[op], (k - 2), (op - 1), (k + op) % 2)
    add(rng.randint(0, 256, (17, 23, 3)), (0.0, 0.0, 0.0), (2, 1, 0), 1.0, 0, 0, 0)
    add(rng.randint(0, 256, (17, 23, 3)), (2.0, 2.0, 2.0), (1, 0, 2), 1.0, 0, 0, 1)
    # a constant image; a 1 x 2 image whose grey mean is exactly 10.5 (m = 11), contrast at 0 shows m itself
    add(np.full((12, 9, 3), 77), (1.3, 0.7, 1.6), (1, 2, 0), 1.01, 1, -1, 0)
    add(np.array([[[10, 10, 10], [11, 11, 11]]]), (1.0, 0.0, 1.0), (0, 1, 2), 1.0, 0, 0, 0)
    add(np.array([[[10, 10, 10], [11, 11, 11]]]), (1.0, 1.1, 1.0), (1, 0, 2), 1.0, 0, 0, 1)
    # dark and bright images: the clamps of the extrapolating blend on both sides
    add(rng.randint(0, 40, (33, 31, 3)), (1.9, 1.8, 1.7), (0, 2, 1), 0.97, -6, 5, 0)
    add(rng.randint(200, 256, (39, 55, 3)), (1.9, 1.8, 0.2), (2, 0, 1), 1.04, 9, -7, 1)
    # everything pushed out: fill only
    add(rng.randint(0, 256, (8, 8, 3)), (1.1, 0.9, 1.1), (0, 1, 2), 1.0, 8, 0, 0)
    return out


def main():
    cs = cases()
    arrays = {}
    for k, (img, factors, order, matrix, swap) in enumerate(cs):
        want = pillow(img, factors, order, matrix, swap)
        got = R.augment(img, factors, order, matrix, swap)
        assert np.array_equal(got, want), f"case {k}: restatement != Pillow"
        arrays[f"in_{k:02d}"], arrays[f"out_{k:02d}"] = img, want
    rng = np.random.RandomState(7)
    for k in range(12):                             # the restatement at the training size
        img = rng.randint(0, 256, (224, 224, 3)).astype(np.uint8)
        factors = (2.0 * rng.rand(), 0.9 + 0.2 * rng.rand(), 0.9 + 0.2 * rng.rand())
        order = rng.permutation(3)
        matrix = R.affine_matrix(224, 224, 0.99 + 0.02 * rng.rand(), int(rng.randint(-2, 3)), int(rng.randint(-2, 3)))
        assert np.array_equal(R.augment(img, factors, order, matrix, k % 2), pillow(img, factors, order, matrix, k % 2)), k
    arrays["factors"] = np.stack([c[1] for c in cs])
    arrays["order"] = np.stack([c[2] for c in cs])
    arrays["matrix"] = np.stack([c[3] for c in cs])
    arrays["swap"] = np.array([c[4] for c in cs], np.int32)
    path = os.path.join(HERE, "color_affine.npz")
    np.savez_compressed(path, **arrays)
    print(f"color_affine: {len(cs)} cases, {os.path.getsize(path)} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
