"""The consensus gaze's oracle and inputs, shared by tests/test_gaze_consensus_{cpu,gpu}.py and scripts/gaze_consensus_bench.py.

``forward`` applies the definition at mvg_gaze_consensus_fwd (include/rotmvgaze.h) literally, item by item, in float64 numpy to
the fp32 inputs; ``backward_autograd`` is float64 torch autograd of a torch restatement of that forward; ``backward_analytic``
restates the header's backward formulas in numpy (the CPU file checks it against autograd).

The bar of the GPU comparisons is derived, not measured: kernel and oracle both compute in double from the same fp32 inputs, so they
differ by one fp32 rounding of the result (half a unit in the last place, at most 2^-24 |ref|) plus double-precision noise, which
the inputs below keep to a single-digit multiple of 1e-16 (|pitch| <= 1.2 bounds asin's conditioning by 1 / cos 1.2 < 2.8, a
resultant >= 0.9 that of the normalisation): |out - ref| <= 2^-24 |ref| + 1e-12 S, S = 1 for head and views, 1 for the resultant,
180 for the spread in degrees, the case's max |ref| for dpreds.
"""
import numpy as np
import torch

CASES = [(1, 2, 1), (3, 2, 5), (3, 3, 300), (2, 8, 5), (3, 4, 300)]      # (iterations, views, batch)
MODES = ("none", "confidence", "mask")
MIN_RESULTANT, MAX_PITCH = 0.9, 1.2
CANCEL = 1e-4                      # |h| <= CANCEL * W: the predictions cancel (a definition)


def bar(ref, scale):
    return 2.0 ** -24 * np.abs(ref) + 1e-12 * scale


def directed(V):
    """(s, q): direction d predicts for view s[d] with partner q[d] (heads.directed_pairs)."""
    s, q = [], []
    for i in range(V):
        for j in range(i + 1, V):
            s += [i, j]
            q += [j, i]
    return s, q


def vec(py):
    p, y = py[..., 0], py[..., 1]
    return np.stack([np.cos(p) * np.sin(y), np.sin(p), np.cos(p) * np.cos(y)], axis=-1)


def rotation(py):
    """(pitch, yaw) [...,2] -> Ry(yaw) @ Rx(-pitch) [...,3,3], float64 (geometry.rotation_matrix_2d's matrix)."""
    p, y = np.asarray(py[..., 0], dtype=np.float64), np.asarray(py[..., 1], dtype=np.float64)
    z, o = np.zeros_like(p), np.ones_like(p)
    ry = np.stack([np.stack([np.cos(y), z, np.sin(y)], -1), np.stack([z, o, z], -1), np.stack([-np.sin(y), z, np.cos(y)], -1)], -2)
    rx = np.stack([np.stack([o, z, z], -1), np.stack([z, np.cos(p), np.sin(p)], -1), np.stack([z, -np.sin(p), np.cos(p)], -1)], -2)
    return ry @ rx


def to_pitchyaw(u):
    return np.stack([np.arcsin(np.clip(u[..., 1], -1.0, 1.0)), np.arctan2(u[..., 0], u[..., 2])], axis=-1)


# ---------------------------------------------------------------- the forward, literally
def _item(preds, rot, w, s, q):
    """One item: preds [D,2], rot [V,3,3], w [V] (float64).  -> (h, W, active [D]) or None when degenerate."""
    D = preds.shape[0]
    if not (np.isfinite(w).all() and (w >= 0).all()):
        return None
    wd = np.array([w[s[d]] * w[q[d]] for d in range(D)])
    active = wd > 0
    if not active.any():
        return None
    h, W = np.zeros(3), 0.0
    for d in range(D):
        if not active[d]:
            continue                                                      # skipped, not multiplied by zero
        if not (np.isfinite(preds[d]).all() and np.isfinite(rot[s[d]]).all()):
            return None
        h = h + wd[d] * (rot[s[d]].T @ vec(preds[d]))
        W = W + wd[d]
    if np.linalg.norm(h) <= CANCEL * W:
        return None
    return h, W, wd, active


def forward(preds, rot, weights=None):
    """preds fp32 [I,D,B,2], rot fp32 [B,V,3,3], weights fp32 [B,V] or None -> float64 head [I,B,3], views [I,V,B,2], stats
    [I,B,2] (resultant length, weighted mean disagreement in degrees); a degenerate item is NaN in all three."""
    preds, rot = np.asarray(preds, dtype=np.float64), np.asarray(rot, dtype=np.float64)
    I, D, B, _ = preds.shape
    V = rot.shape[1]
    assert D == V * (V - 1)
    s, q = directed(V)
    w = np.ones((B, V)) if weights is None else np.asarray(weights, dtype=np.float64)
    head, views, stats = np.full((I, B, 3), np.nan), np.full((I, V, B, 2), np.nan), np.full((I, B, 2), np.nan)
    with np.errstate(invalid="ignore"):
        for it in range(I):
            for b in range(B):
                r = _item(preds[it, :, b], rot[b], w[b], s, q)
                if r is None:
                    continue
                h, W, wd, active = r
                n = np.linalg.norm(h)
                e = h / n
                head[it, b] = e
                for t in range(V):
                    if np.isfinite(rot[b, t]).all():                      # (a non-finite rot[b][t]: a NaN row for that t only)
                        views[it, t, b] = to_pitchyaw(rot[b, t] @ e)
                ang = sum(wd[d] * np.arccos(np.clip(e @ (rot[b, s[d]].T @ vec(preds[it, d, b])), -1.0, 1.0)) for d in range(D) if active[d])
                stats[it, b] = (n / W, ang * 180.0 / np.pi / W)
    return head, views, stats


# ---------------------------------------------------------------- the backward: the header's formulas, and autograd
def backward_analytic(dviews, preds, rot, weights=None):
    """The backward formulas at mvg_gaze_consensus_bwd, item by item in float64 numpy -> dpreds [I,D,B,2]."""
    dviews, preds, rot = (np.asarray(a, dtype=np.float64) for a in (dviews, preds, rot))
    I, D, B, _ = preds.shape
    V = rot.shape[1]
    s, q = directed(V)
    w = np.ones((B, V)) if weights is None else np.asarray(weights, dtype=np.float64)
    out = np.zeros((I, D, B, 2))
    for it in range(I):
        for b in range(B):
            r = _item(preds[it, :, b], rot[b], w[b], s, q)
            if r is None:
                continue
            h, W, wd, active = r
            n = np.linalg.norm(h)
            e = h / n
            ge = np.zeros(3)
            for t in range(V):
                if not np.isfinite(rot[b, t]).all():
                    continue
                u = rot[b, t] @ e
                r2 = u[0] * u[0] + u[2] * u[2]
                if r2 == 0.0 or u[1] * u[1] >= 1.0:
                    continue
                dp, dy = dviews[it, t, b]
                ge = ge + rot[b, t].T @ np.array([dy * u[2] / r2, dp / np.sqrt(1.0 - u[1] * u[1]), -dy * u[0] / r2])
            gh = (ge - (ge @ e) * e) / n
            for d in range(D):
                if not active[d]:
                    continue
                gv = wd[d] * (rot[b, s[d]] @ gh)
                p, y = preds[it, d, b]
                out[it, d, b, 0] = gv @ np.array([-np.sin(p) * np.sin(y), np.cos(p), -np.sin(p) * np.cos(y)])
                out[it, d, b, 1] = gv @ np.array([np.cos(p) * np.cos(y), 0.0, -np.cos(p) * np.sin(y)])
    return out


def backward_autograd(dviews, preds, rot, weights=None):
    """d sum(dviews * views) / d preds by float64 torch autograd of the forward restated in torch (vectorised over the items;
    skipped entries are replaced by constants BEFORE the arithmetic, so nothing non-finite enters the graph).  Which items are
    degenerate and which contributions are active comes from ``forward`` / the weights, as the definition has it."""
    preds64, rot64 = np.asarray(preds, dtype=np.float64), np.asarray(rot, dtype=np.float64)
    I, D, B, _ = preds64.shape
    V = rot64.shape[1]
    s, q = directed(V)
    w = np.ones((B, V)) if weights is None else np.asarray(weights, dtype=np.float64)
    head, views, _ = forward(preds, rot, weights)
    ok_item = np.isfinite(head).all(-1)                                   # [I,B]
    with np.errstate(invalid="ignore"):
        wd = np.nan_to_num(w[:, s] * w[:, q], nan=0.0, posinf=0.0, neginf=0.0).T          # [D,B]
    active = (wd > 0)[None] & ok_item[:, None]                            # [I,D,B]
    ok_target = np.isfinite(views).all(-1)                                # [I,V,B]
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    p = T(np.where(active[..., None], preds64, 0.0)).requires_grad_(True)
    wt = T(np.where(active, wd[None], 0.0))                               # [I,D,B]
    used = active.any(0)                                                  # [D,B]: the source rot is finite wherever it is used
    rs = T(np.where(used[..., None, None], np.moveaxis(rot64[:, s], 0, 1), 0.0))          # [D,B,3,3]
    rt = T(np.where(np.isfinite(rot64).all((-1, -2))[..., None, None], rot64, np.eye(3)))  # [B,V,3,3]
    v = torch.stack([torch.cos(p[..., 0]) * torch.sin(p[..., 1]), torch.sin(p[..., 0]), torch.cos(p[..., 0]) * torch.cos(p[..., 1])], -1)
    hv = torch.einsum("dbkm,idbk->idbm", rs, v)
    h = (wt[..., None] * hv).sum(1)                                       # [I,B,3]
    h = torch.where(T(ok_item)[..., None], h, torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64))
    e = h / h.norm(dim=-1, keepdim=True)
    u = torch.einsum("btkm,ibm->itbk", rt, e)                             # [I,V,B,3]
    keep = T(ok_target) & (u[..., 1] ** 2 < 1).detach() & ((u[..., 0] ** 2 + u[..., 2] ** 2) > 0).detach()
    uy = torch.where(keep, u[..., 1], torch.zeros((), dtype=torch.float64))
    ux = torch.where(keep, u[..., 0], torch.zeros((), dtype=torch.float64))
    uz = torch.where(keep, u[..., 2], torch.ones((), dtype=torch.float64))
    out = torch.stack([torch.asin(uy), torch.atan2(ux, uz)], -1)
    g = T(np.where(keep.numpy()[..., None], np.asarray(dviews, dtype=np.float64), 0.0))
    (out * g).sum().backward()
    return p.grad.numpy()


# ---------------------------------------------------------------- inputs
def make_inputs(I, V, B, seed, noise=0.05, dtype=np.float32):
    """Head poses and one head-frame gaze per sample from U(-0.5, 0.5) rad; each prediction is that gaze rotated into its view
    plus N(0, noise^2).  fp32 (the kernels' inputs; dtype=np.float64 for the oracle's self-checks): preds [I,D,B,2], rot [B,V,3,3]."""
    rng = np.random.default_rng(seed)
    s, _ = directed(V)
    rot = rotation(rng.uniform(-0.5, 0.5, size=(B, V, 2)))                # float64 [B,V,3,3]
    gaze = vec(rng.uniform(-0.5, 0.5, size=(B, 2)))                       # head frame [B,3]
    in_view = to_pitchyaw(np.einsum("bvkm,bm->bvk", rot, gaze))          # [B,V,2]
    preds = np.moveaxis(in_view[:, s], 0, 1)[None] + rng.normal(0.0, noise, size=(I, len(s), B, 2))
    return preds.astype(dtype), rot.astype(dtype)


def make_weights(mode, V, B, seed):
    """None | confidences in [0.25, 2] | confidences with one view of every third sample at 0 (never below two active views)."""
    if mode == "none":
        return None
    rng = np.random.default_rng(seed + 1000)
    w = rng.uniform(0.25, 2.0, size=(B, V)).astype(np.float32)
    if mode == "mask" and V > 2:
        for b in range(0, B, 3):
            w[b, rng.integers(V)] = 0.0
    return w


def check_conditioning(preds, rot, weights, planted=()):
    """Every non-planted item of a case: resultant >= 0.9 and |pitch| <= 1.2 (what the derived bar assumes).  planted: (it, b)."""
    _, views, stats = forward(preds, rot, weights)
    keep = np.ones(stats.shape[:2], dtype=bool)
    for it, b in planted:
        keep[it, b] = False
    assert len(planted) * 8 <= keep.size or not planted
    assert np.isfinite(stats[keep]).all() and stats[keep][:, 0].min() >= MIN_RESULTANT, stats[keep][:, 0].min()
    fin = np.isfinite(views[..., 0])
    assert np.abs(views[..., 0][fin]).max() <= MAX_PITCH and np.abs(np.asarray(preds)[..., 0][np.isfinite(np.asarray(preds)[..., 0])]).max() <= MAX_PITCH
