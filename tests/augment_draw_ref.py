"""NumPy restatement of mvg_augment_draw (include/rotmvgaze.h): Philox4x32-10 and the whole per-image draw, float32 and
float64 operations one at a time in the order the header gives, so that the device's buffers can be compared bit for bit.
Independent of rot_mvgaze_amd: the settings are TrainAugment's constructor arguments, restated here."""
import numpy as np

REC = np.dtype([("factor", np.float32, 3), ("order", np.int32, 3), ("a0", np.float64), ("cx", np.float64), ("a4", np.float64),
                ("cy", np.float64)], align=True)
PERMS = np.array([(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)], np.int32)       # lexicographic
RECIPE = dict(brightness=1.0, contrast=0.1, saturation=0.1, scale=(0.99, 1.01), translate=(0.01, 0.01),
              erase=dict(p=0.5, proportion=(0.5, 0.6), dot_size=(0.05, 0.3)))                          # the reference's (main.py:41-49)
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: uint32 [..., 4]; key: two 32-bit words -> uint32 [..., 4]."""
    c = [np.asarray(counter, np.uint32)[..., k].astype(np.uint64) for k in range(4)]
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, -1).astype(np.uint32)


def u01(x):
    """float(x >> 8) * 2^-24: exact in float32."""
    return (np.asarray(x, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def _range(value):
    """ColorJitter's [max(0, 1 - v), 1 + v] as float32; a disabled op (v == 0) is [1, 1]."""
    return np.float32(max(0.0, 1.0 - float(value))), np.float32(1.0 + float(value))


def _uniform32(x, lo, hi):
    return u01(x) * (np.float32(hi) - np.float32(lo)) + np.float32(lo)           # float32 ops, each rounded


def _uniform64(x, lo, hi):
    return np.float64(lo) + (np.float64(hi) - np.float64(lo)) * u01(x).astype(np.float64)


def gmax_of(erase):
    return 0 if erase is None else int(1.0 / float(erase["dot_size"][0]))


def draw(n, h, w, seed, counter, brightness=1.0, contrast=0.1, saturation=0.1, scale=(0.99, 1.01), translate=(0.01, 0.01), erase=None):
    """-> (recs [n] REC, masks float32 [n, gmax*gmax] or None, grid int32 [n] or None, extras): what launch number
    `counter` of a TrainAugment(draws="device", seed=seed) with these settings writes.  extras: tx, ty, the float32 scale, and
    prop / the erase decision, for the distribution tests."""
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    c2, c3 = counter & 0xFFFFFFFF, (counter >> 32) & 0xFFFFFFFF

    def blocks(i, j):
        i, j = np.broadcast_arrays(np.asarray(i, np.uint32), np.asarray(j, np.uint32))
        ctr = np.stack([i, j, np.full(i.shape, c2, np.uint32), np.full(i.shape, c3, np.uint32)], -1)
        return philox4x32_10(ctr, key)

    idx = np.arange(n, dtype=np.uint32)
    b0, b1, b2 = blocks(idx, 0), blocks(idx, 1), blocks(idx, 2)
    recs = np.zeros(n, REC)
    k = ((b0[:, 0].astype(np.uint64) * np.uint64(6)) >> np.uint64(32)).astype(np.int64)
    recs["order"] = PERMS[k]
    for op, v in enumerate((brightness, contrast, saturation)):
        lo, hi = _range(v)
        recs["factor"][:, op] = _uniform32(b0[:, 1 + op], lo, hi)
    max_dx = np.float32(float(translate[0] * w)) if translate is not None else np.float32(0.0)
    max_dy = np.float32(float(translate[1] * h)) if translate is not None else np.float32(0.0)
    tx = np.rint(u01(b1[:, 0]) * (np.float32(2.0) * max_dx) - max_dx).astype(np.int32)             # half to even
    ty = np.rint(u01(b1[:, 1]) * (np.float32(2.0) * max_dy) - max_dy).astype(np.int32)
    s32 = _uniform32(b1[:, 2], *(scale if scale is not None else (1.0, 1.0)))
    assert s32.dtype == np.float32 and recs["factor"].dtype == np.float32
    a0 = np.float64(1.0) / s32.astype(np.float64)
    x0, y0 = np.float64(w) * 0.5, np.float64(h) * 0.5
    recs["a0"], recs["a4"] = a0, a0
    recs["cx"] = a0 * (-x0 - tx.astype(np.float64)) + x0
    recs["cy"] = a0 * (-y0 - ty.astype(np.float64)) + y0
    extras = dict(tx=tx, ty=ty, scale=s32)
    if erase is None:
        return recs, None, None, extras
    gmax = gmax_of(erase)
    cells = gmax * gmax
    applied = ~(u01(b1[:, 3]).astype(np.float64) > np.float64(erase["p"]))
    dot = _uniform64(b2[:, 0], *erase["dot_size"])
    g = np.clip((np.float64(1.0) / dot).astype(np.int64), 1, gmax)
    prop = _uniform64(b2[:, 1], *erase["proportion"])
    grid = np.where(applied, g, 0).astype(np.int32)
    nblk = (cells + 3) // 4
    words = blocks(idx[:, None], 3 + np.arange(nblk, dtype=np.uint32)[None, :]).reshape(n, nblk * 4)[:, :cells]
    keep = u01(words).astype(np.float64) > prop[:, None]
    inside = np.arange(cells)[None, :] < (grid.astype(np.int64) ** 2)[:, None]
    masks = np.where(keep & inside, np.float32(1.0), np.float32(0.0)).astype(np.float32)
    extras.update(prop=prop, applied=applied)
    return recs, masks, grid, extras
