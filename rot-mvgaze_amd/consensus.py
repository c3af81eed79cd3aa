"""Multi-view consensus gaze: one estimate per sample from all V (V - 1) directed pair predictions.

The model predicts once per directed pair, each prediction in the camera frame of the view it was made for.  Its own premise -
views relate through the head-pose rotations, ``rel = rot_i @ rot_j^T`` - also maps every prediction into the head frame
(``rot[b][s]^T v``), where predictions can be averaged: ``gaze_consensus`` sums the (confidence-weighted) head-frame unit vectors,
normalises the resultant and rotates it back into every view.  A view with weight 0 is missing: its contributions are skipped
(not multiplied by zero), and it still receives the consensus in its own frame.  The definition, with the degenerate cases, is at
``mvg_gaze_consensus_fwd`` in include/rotmvgaze.h; forward and backward are one library launch each, in double, with no
synchronisation (legal inside ``torch.cuda.graph``).

There is no CPU fallback: host tensors raise.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops

Tensor = torch.Tensor


def _check(preds: Tensor, rot: Tensor, weights: Optional[Tensor]):
    if not (isinstance(preds, Tensor) and isinstance(rot, Tensor) and preds.is_cuda and rot.is_cuda
            and (weights is None or (isinstance(weights, Tensor) and weights.is_cuda))):
        raise RuntimeError("gaze_consensus: the MI355X path needs device tensors (no CPU fallback)")
    if preds.dim() != 4 or preds.shape[3] != 2 or rot.dim() != 4 or tuple(rot.shape[2:]) != (3, 3):
        raise ValueError(f"gaze_consensus: expected preds [I,D,B,2] and rot [B,V,3,3], got {tuple(preds.shape)} and {tuple(rot.shape)}")
    I, D, B = preds.shape[0], preds.shape[1], preds.shape[2]
    V = rot.shape[1]
    if rot.shape[0] != B or D != V * (V - 1):
        raise ValueError(f"gaze_consensus: preds {tuple(preds.shape)} are not the V (V - 1) directed pairs of rot {tuple(rot.shape)}")
    if weights is not None and tuple(weights.shape) != (B, V):
        raise ValueError(f"gaze_consensus: weights must be [B,V] = {(B, V)}, got {tuple(weights.shape)}")
    return I, V, B


class _ConsensusFn(torch.autograd.Function):
    """(head, views, stats or None) of mvg_gaze_consensus_fwd; the gradient flows from ``views`` to ``preds`` only."""

    @staticmethod
    def forward(ctx, preds: Tensor, rot: Tensor, weights: Optional[Tensor], stats: bool):
        I, V, B = _check(preds, rot, weights)
        p = preds.detach().to(torch.float32).contiguous()
        r = rot.detach().to(torch.float32).contiguous()
        w = weights.detach().to(torch.float32).contiguous() if weights is not None else None
        mk = lambda *s: torch.empty(*s, dtype=torch.float32, device=p.device)
        head, views, st = mk(I, B, 3), mk(I, V, B, 2), (mk(I, B, 2) if stats else None)
        with torch.cuda.device(p.device):
            ops.gaze_consensus_fwd(p, r, w, I, V, B, head, views, st)
        ctx.mvg = (p, r, w, I, V, B) if ctx.needs_input_grad[0] else None
        ctx.mark_non_differentiable(*((head,) if st is None else (head, st)))
        return head, views, st

    @staticmethod
    def backward(ctx, _ghead, gviews, _gstats):
        if ctx.mvg is None or gviews is None:
            return None, None, None, None
        p, r, w, I, V, B = ctx.mvg
        dpreds = torch.empty_like(p)
        with torch.cuda.device(p.device):
            ops.gaze_consensus_bwd(gviews.to(torch.float32).contiguous(), p, r, w, I, V, B, dpreds)
        return dpreds, None, None, None


def gaze_consensus(preds: Tensor, rot: Tensor, weights: Optional[Tensor] = None, stats: bool = False):
    """preds ``[I,D,B,2]`` (the heads' stacked buffer, ``heads.directed_pairs`` order), rot ``[B,V,3,3]``, weights ``[B,V]`` or
    None (all 1) -> ``(head [I,B,3], views [I,V,B,2])``, and with ``stats=True`` a third ``[I,B,2]``: the resultant length in
    [0, 1] and the weighted mean disagreement in degrees.  A degenerate item (no active contribution, a negative or non-finite
    weight, a non-finite active input, cancelling predictions) is NaN in every output and has zero gradient."""
    head, views, st = _ConsensusFn.apply(preds, rot, weights, bool(stats))
    return (head, views, st) if stats else (head, views)
