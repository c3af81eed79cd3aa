"""Test helper (not collected, not imported by the package): the two operand layouts of the bf16 stem, restated in NumPy
for an image that is already rounded to bf16 (any integer or float dtype: the helper only moves values and writes zeros;
the tests pass the bf16 bit patterns as int16).

    NHWC8        x8[i, y, x, c] = img[i, y, x, c] for c < 3, else 0
    row windows  xw[i, y, m, 4 j + c] = img[i, y, 4 m - 4 + j, c] for 0 <= 4 m - 4 + j < w and c < 3, else 0
                 (m < w / 4, j < 16: window m of an image row holds columns 4 m - 4 .. 4 m + 11, four stored channels each)
"""
import numpy as np


def nhwc8(img):
    n, h, w = img.shape[:3]
    out = np.zeros((n, h, w, 8), dtype=img.dtype)
    out[..., :3] = img[..., :3]
    return out


def row_windows(img):
    n, h, w = img.shape[:3]
    assert w % 4 == 0 and img.shape[3] >= 3
    padded = np.zeros((n, h, w + 12, 4), dtype=img.dtype)          # columns -4 .. w + 7
    padded[:, :, 4:4 + w, :3] = img[..., :3]
    out = np.zeros((n, h, w // 4, 64), dtype=img.dtype)
    for m in range(w // 4):
        out[:, :, m] = padded[:, :, 4 * m:4 * m + 16].reshape(n, h, 64)
    return out
