"""Test helper (not collected, not imported by the package): ColorJitter (brightness, contrast, saturation) and the
scale / translate RandomAffine of the reference's training transform (main.py:41-49) on one uint8 HWC image, restated
in NumPy from what torchvision runs on a PIL image - ImageEnhance.{Brightness, Contrast, Color} (ImagingBlend) and
Image.transform(AFFINE, NEAREST) (ImagingScaleAffine).  tests/golden/make_golden_augment.py holds it against Pillow
itself.  The steps run in Pillow's order - the three enhance ops over the whole image, each quantised to uint8, then the
gather - not in the kernel's (gather first), so agreement also checks that the two orders are the same thing.

    grey      L = (R*19595 + G*38470 + B*7471 + 0x8000) >> 16
    blend     t = deg + f*(pix - deg) in float32, f rounded to float32; 0 <= f <= 1: t truncated, else clamped to
              0 / 255 where t <= 0 / t >= 255 and truncated between
    degenerate image: brightness 0; saturation L of the pixel; contrast m = int(S / N + 0.5), S the sum of L over the
              image as it stands when contrast runs, N = h*w
    gather    per axis o = c + a*0.5, then for each output index src = -1 if o < 0 else int(o), o += a (the SAME
              repeated double additions); src outside [0, size) = fill (0)
"""
import numpy as np

BRIGHTNESS, CONTRAST, SATURATION = 0, 1, 2


def grey(rgb):
    v = rgb.astype(np.int64)
    return (v[..., 0] * 19595 + v[..., 1] * 38470 + v[..., 2] * 7471 + 0x8000) >> 16


def blend(deg, pix, f):
    f = np.float32(f)
    d, p = deg.astype(np.float32), pix.astype(np.float32)
    t = d + f * (p - d)                      # float32 throughout, one rounding per operation
    assert t.dtype == np.float32
    if np.float32(0) <= f <= np.float32(1):
        return t.astype(np.int64).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int64))).astype(np.uint8)


def contrast_mean(rgb):
    g = grey(rgb)
    return int(float(int(g.sum())) / float(g.size) + 0.5)


def enhance(rgb, op, f):
    """One ImageEnhance op on an RGB uint8 [h, w, 3] image."""
    if op == BRIGHTNESS:
        deg = np.zeros_like(rgb)
    elif op == CONTRAST:
        deg = np.full_like(rgb, contrast_mean(rgb))
    elif op == SATURATION:
        deg = np.repeat(grey(rgb)[..., None], 3, axis=-1)
    else:
        raise ValueError(op)
    return blend(deg, rgb, f)


def axis_table(size, a, c):
    tab, o = [], c + a * 0.5
    for _ in range(size):
        s = -1 if o < 0.0 else int(o)
        tab.append(s if s < size else -1)
        o += a
    return np.array(tab, dtype=np.int64)


def gather(rgb, a0, cx, a4, cy):
    h, w = rgb.shape[:2]
    xt, yt = axis_table(w, a0, cx), axis_table(h, a4, cy)
    out = rgb[np.clip(yt, 0, h - 1)][:, np.clip(xt, 0, w - 1)].copy()
    out[yt < 0, :] = 0
    out[:, xt < 0] = 0
    return out


def affine_matrix(h, w, scale, tx, ty):
    """torchvision's inverse matrix for angle 0, no shear, centre (w/2, h/2), in Python doubles: (a0, c_x, a4, c_y)."""
    cx, cy = w * 0.5, h * 0.5
    a0 = a4 = 1.0 / scale
    return a0, a0 * (-cx - tx) + cx, a4, a4 * (-cy - ty) + cy


def augment(u8, factors, order, matrix, swap_rb=False):
    """u8 [h, w, 3] -> uint8 [h, w, 3] RGB: optional B/R swap, the three ops in `order` (a permutation of
    BRIGHTNESS, CONTRAST, SATURATION; factors indexed by op), then the gather."""
    img = np.ascontiguousarray(u8[..., ::-1] if swap_rb else u8)
    assert sorted(int(o) for o in order) == [0, 1, 2]
    for op in order:
        img = enhance(img, int(op), factors[int(op)])
    return gather(img, *[float(m) for m in matrix])
