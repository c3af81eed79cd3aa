"""Gaze error meter: the number the trainer prints, accumulated on the device in float64 and read once per epoch.

The reference leaves the device for its metric: once per training step (/root/reference/trainer.py:128,
``np.mean(angular_error(pred_gaze.cpu()..., gt.cpu()...))``) and once per test batch (trainer.py:187-192) - a device-to-host copy
and a pipeline drain each.  ``AngularErrorMeter`` keeps the same quantity - utils/math.py:105-120 in double, per (iteration,
direction) cell: count, sum, sum of squares, maximum, and the rows with a NaN / Inf input - in a small device record that
``update`` adds to with ONE library launch (``mvg_gaze_error_update``; no synchronisation, legal inside ``torch.cuda.graph`` and
inside ``GraphedStep``'s ``step_fn``) and ``compute`` reads with one copy.  With ``capacity > 0`` the per-sample errors are kept
too (the device form of ``pred_gaze_all`` / ``gt_gaze_all``, trainer.py:169-189) for medians and percentiles on the host.

The one deviation from the reference's formula: the similarity is clamped to [-1, 1] before ``acos`` - a prediction equal to its
label gives 0 here, where the reference's float64 similarity can round to 1 + 2e-16 and return NaN.

There is no CPU fallback: ``update`` on host tensors raises.
"""
from __future__ import annotations

from typing import Any, Dict, Optional

import numpy as np
import torch

from . import ops
from ._lib import GAZE_ERR_COUNT, GAZE_ERR_FIELDS, GAZE_ERR_MAX, GAZE_ERR_NONFINITE, GAZE_ERR_SUM, GAZE_ERR_SUMSQ
from .heads import directed_pairs

Tensor = torch.Tensor


def build_gt_dir(gt: Tensor, views: int) -> Tensor:
    """gt [B,V,2] -> fp32 [D,B,2]: row d holds the labels of the view direction d predicts for (``directed_pairs``), the layout
    ``MultiViewIterationLoss`` builds.  Slices, not ``gt[:, vi]``: indexing with a Python list builds the index tensor on the host
    and its copy to the device waits for the stream - a synchronisation per batch."""
    if gt.dim() != 3 or gt.shape[1] != views or gt.shape[2] != 2:
        raise ValueError(f"gt must be [B, {views}, 2], got {tuple(gt.shape)}")
    vi, _ = directed_pairs(views)
    g32 = gt.to(torch.float32)
    return torch.stack([g32[:, v] for v in vi], 0)


class AngularErrorMeter:
    """``AngularErrorMeter(num_iter=1, dirs=1, capacity=0, device=None, output_index=-1)``.

    num_iter, dirs: the cells of the record - the model's iterations and directed pairs V (V - 1) (2 for the two-view model; 1, 1
    for plain ``[N,2]`` tensors).  capacity: per-sample errors kept per cell (0: none).  device: where the record lives (None: the
    device of the first ``update``).  output_index: the iteration ``error_gaze`` reports (the model's ``_output_index``).

    ``update`` takes one of
      ``update(data)``       the dict ``FeatRotationSymm.forward`` returned (``_mvg_preds``, ``gt_gaze``, ``gt_gaze_1``);
      ``update(out, gt)``    the dict of ``forward_multiview`` and gt ``[B,V,2]``;
      ``update(pred, gt)``   device tensors ``[N,2]`` (one cell).
    ``update_consensus(out, gt)`` (a meter with ``dirs = V``) takes the consensus gaze of ``forward_multiview(..., consensus=True)``.
    Inside a captured step the eager warm-up steps of ``GraphedStep`` count like any other update (the capture pass itself runs
    nothing): call ``reset()`` after building the graph (stream-ordered, so it lands before the first replay)."""

    def __init__(self, num_iter: int = 1, dirs: int = 1, capacity: int = 0, device=None, output_index: int = -1) -> None:
        if num_iter < 1 or dirs < 1 or capacity < 0:
            raise ValueError("AngularErrorMeter: num_iter and dirs must be >= 1, capacity >= 0")
        if not -num_iter <= output_index < num_iter:
            raise ValueError(f"AngularErrorMeter: output_index {output_index} outside {num_iter} iterations")
        self.num_iter, self.dirs, self.capacity, self.output_index = int(num_iter), int(dirs), int(capacity), int(output_index)
        self.record: Optional[Tensor] = None        # float64 [I, D, GAZE_ERR_FIELDS]
        self.err_out: Optional[Tensor] = None       # fp32 [I, D, capacity]
        if device is not None:
            self._ensure(torch.device(device))

    def _ensure(self, device: torch.device) -> None:
        if device.type != "cuda":
            raise RuntimeError("AngularErrorMeter: the MI355X path needs device tensors (no CPU fallback)")
        if self.record is None:
            self.record = torch.zeros(self.num_iter, self.dirs, GAZE_ERR_FIELDS, dtype=torch.float64, device=device)
            if self.capacity:
                self.err_out = torch.empty(self.num_iter, self.dirs, self.capacity, dtype=torch.float32, device=device)
        elif self.record.device != device:
            raise RuntimeError(f"AngularErrorMeter: the record lives on {self.record.device}, the update is on {device}")

    # ---------------------------------------------------------------- accumulate
    def update(self, a: Any, gt: Optional[Tensor] = None) -> None:
        if isinstance(a, dict):
            preds = a.get("_mvg_preds")
            if preds is None:
                raise ValueError("AngularErrorMeter.update: the dict holds no '_mvg_preds' (not an output of this package's model)")
            if gt is None:
                gt_dir = torch.stack([a["gt_gaze"], a["gt_gaze_1"]], 0).to(torch.float32)
            else:
                gt_dir = build_gt_dir(gt, int(a["views"]))
        else:
            if gt is None or not isinstance(a, Tensor) or a.dim() != 2 or a.shape[1] != 2 or tuple(gt.shape) != tuple(a.shape):
                raise ValueError("AngularErrorMeter.update: expected update(pred [N,2], gt [N,2]), update(dict) or update(dict, gt [B,V,2])")
            preds, gt_dir = a.reshape(1, 1, -1, 2), gt.reshape(1, -1, 2)
        if not (isinstance(preds, Tensor) and preds.is_cuda and gt_dir.is_cuda):
            raise RuntimeError("AngularErrorMeter: the MI355X path needs device tensors (no CPU fallback)")
        I, D, B = preds.shape[0], preds.shape[1], preds.shape[2]
        if (I, D) != (self.num_iter, self.dirs) or tuple(gt_dir.shape) != (D, B, 2):
            raise ValueError(f"AngularErrorMeter: made for {self.num_iter} iterations x {self.dirs} directions, got predictions "
                             f"{tuple(preds.shape)} and labels {tuple(gt_dir.shape)}")
        self._ensure(preds.device)
        p = preds.detach().to(torch.float32).contiguous()
        g = gt_dir.detach().to(torch.float32).contiguous()
        with torch.cuda.device(p.device):
            ops.gaze_error_update(p, g, I, D, B, self.record, self.err_out, self.capacity)

    def update_consensus(self, out: Dict[str, Any], gt: Tensor) -> None:
        """For a meter made with ``dirs = V``: adds the errors of the consensus gaze (``out["consensus"]["views"]`` [I,V,B,2] of
        ``forward_multiview(..., consensus=True)``) against gt [B,V,2] - cell (it, t) is view t.  One ``mvg_gaze_error_update``;
        a degenerate sample (NaN consensus) counts in ``nonfinite``."""
        cons = out.get("consensus") if isinstance(out, dict) else None
        if cons is None:
            raise ValueError("AngularErrorMeter.update_consensus: the dict holds no 'consensus' (forward_multiview(..., consensus=True))")
        views = cons["views"]
        if not (isinstance(views, Tensor) and views.is_cuda and isinstance(gt, Tensor) and gt.is_cuda):
            raise RuntimeError("AngularErrorMeter: the MI355X path needs device tensors (no CPU fallback)")
        I, V, B = views.shape[0], views.shape[1], views.shape[2]
        if (I, V) != (self.num_iter, self.dirs) or tuple(gt.shape) != (B, V, 2):
            raise ValueError(f"AngularErrorMeter: made for {self.num_iter} iterations x {self.dirs} views, got consensus views "
                             f"{tuple(views.shape)} and labels {tuple(gt.shape)}")
        self._ensure(views.device)
        p = views.detach().to(torch.float32).contiguous()
        g = gt.detach().to(torch.float32).transpose(0, 1).contiguous()
        with torch.cuda.device(p.device):
            ops.gaze_error_update(p, g, I, V, B, self.record, self.err_out, self.capacity)

    def reset(self) -> None:
        """Back to the empty record (a stream-ordered fill; the stored per-sample errors are trimmed by the counters)."""
        if self.record is not None:
            self.record.zero_()

    # ---------------------------------------------------------------- read (synchronises: one device-to-host copy)
    def compute(self) -> Dict[str, Any]:
        """``error_gaze``: the mean error of cell (output_index, direction 0), what trainer.py:128/192 prints - NaN when a row of
        that cell was non-finite, as the reference's mean would be.  ``mean`` / ``std`` / ``max`` / ``count`` / ``nonfinite``: numpy
        ``[num_iter, dirs]`` (mean and std NaN for an empty cell; std is the population form, ``np.std``)."""
        if self.record is None:
            rec = np.zeros((self.num_iter, self.dirs, GAZE_ERR_FIELDS))
        else:
            rec = self.record.cpu().numpy()
        count, nonfinite = rec[..., GAZE_ERR_COUNT], rec[..., GAZE_ERR_NONFINITE]
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = rec[..., GAZE_ERR_SUM] / count
            std = np.sqrt(np.maximum(rec[..., GAZE_ERR_SUMSQ] / count - mean * mean, 0.0))
        o = self.output_index
        return {"error_gaze": float("nan") if nonfinite[o, 0] > 0 else float(mean[o, 0]),
                "mean": mean, "std": std, "max": rec[..., GAZE_ERR_MAX].copy(),
                "count": count.astype(np.int64), "nonfinite": nonfinite.astype(np.int64)}

    def errors(self) -> np.ndarray:
        """The stored per-sample errors, fp32 numpy ``[num_iter, dirs, n]``, n = rows seen (at most ``capacity``; ``overflowed()``
        says whether rows were dropped).  NaN marks a non-finite row."""
        if not self.capacity:
            raise RuntimeError("AngularErrorMeter: made with capacity=0, no per-sample errors are kept")
        if self.record is None:
            return np.zeros((self.num_iter, self.dirs, 0), dtype=np.float32)
        seen = self._seen()
        return self.err_out[:, :, :min(seen, self.capacity)].cpu().numpy()

    def overflowed(self) -> bool:
        """More rows were seen than ``capacity`` holds (the counters went on, the store did not)."""
        return self.record is not None and self._seen() > self.capacity

    def _seen(self) -> int:
        cell = self.record[0, 0].cpu().numpy()       # every cell sees the same rows
        return int(cell[GAZE_ERR_COUNT] + cell[GAZE_ERR_NONFINITE])
