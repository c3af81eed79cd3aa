"""The gaze error meter's oracle and inputs, shared by tests/test_gaze_error_{cpu,gpu}.py and scripts/eval_metric_bench.py's check.

The oracle is ``rot_mvgaze_amd.geometry.angular_error`` on float64 numpy arrays (the reference's evaluation metric,
utils/math.py:105-120, pinned to the reference's fixtures by tests/test_cabi_cpu.py::test_host_angular_error_metric) with the
meter's one documented deviation: the similarity clamped to [-1, 1] before acos.  ``angular_error`` has no hook for the clamp,
so ``oracle`` restates its last line over the same vectors and is checked against it wherever the clamp is inactive
(``test_oracle_is_the_host_metric`` in the CPU file).
"""
import numpy as np

PER_ELEMENT_BAR_DEG = 1e-8         # |device - oracle| on the double path, rows with an oracle error >= FLOOR_DEG
FLOOR_DEG = 0.01                   # rows below it are outside the per-element bar (acos near 1: the conditioning, not the library)
MAX_EXCLUDED = 0.01                # at most this fraction of the rows may fall below the floor
SHAPES = [(1, 1, 1), (3, 2, 5), (3, 2, 300), (2, 6, 64)]       # (iterations, directions, batch)


def _vec(x):
    s, c = np.sin(x), np.cos(x)
    return np.stack([c[:, 0] * s[:, 1], s[:, 0], c[:, 0] * c[:, 1]], axis=1)


def oracle(pred, gt):
    """Degrees, float64 [N]: angular_error's formula (pitch/yaw rows [N,2], widened to float64) with the clamp."""
    a, b = _vec(np.asarray(pred, dtype=np.float64)), _vec(np.asarray(gt, dtype=np.float64))
    ab = np.sum(a * b, axis=1)
    na = np.clip(np.linalg.norm(a, axis=1), 1e-7, None)
    nb = np.clip(np.linalg.norm(b, axis=1), 1e-7, None)
    return np.arccos(np.clip(ab / (na * nb), -1.0, 1.0)) * 180.0 / np.pi


def oracle_cells(preds, gt_dir):
    """preds [I,D,B,2], gt_dir [D,B,2] -> float64 [I,D,B]."""
    I, D, B, _ = preds.shape
    return np.stack([np.stack([oracle(preds[i, d], gt_dir[d]) for d in range(D)]) for i in range(I)])


def make_inputs(I, D, B, seed):
    """gt uniform in +-1.2 rad; pred = gt + a perturbation of log-uniform magnitude from 0.015 deg to about 57 deg (1 rad) in a
    uniformly random direction of the (pitch, yaw) plane.  fp32 arrays: preds [I,D,B,2], gt_dir [D,B,2]."""
    rng = np.random.default_rng(seed)
    gt = rng.uniform(-1.2, 1.2, size=(D, B, 2))
    mag = np.exp(rng.uniform(np.log(np.deg2rad(0.015)), np.log(1.0), size=(I, D, B)))
    phi = rng.uniform(0.0, 2.0 * np.pi, size=(I, D, B))
    preds = gt[None] + mag[..., None] * np.stack([np.cos(phi), np.sin(phi)], axis=-1)
    return preds.astype(np.float32), gt.astype(np.float32)


def record_of(errors):
    """The record cell (COUNT, SUM, SUMSQ, MAX, NONFINITE) of float64 per-row errors [..., N] (NaN = a non-finite row)."""
    ok = np.isfinite(errors)
    e = np.where(ok, errors, 0.0)
    return np.stack([ok.sum(-1).astype(np.float64), e.sum(-1), (e * e).sum(-1), e.max(-1, initial=0.0), (~ok).sum(-1).astype(np.float64)], -1)
