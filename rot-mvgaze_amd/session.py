"""Inference session: the whole eval-mode forward queued by ONE call into librotmvgaze_hip.so.

``InferenceSession`` is the Python face of the handle-level C ABI (``mvg_session_*`` in include/rotmvgaze.h): a plan built
on the host for one (architecture, V, B, H, W) shape, a caller-owned workspace, and a forward that queues the same entry
points ``MultiViewGaze.run_views`` calls under ``model.eval()`` / ``torch.no_grad()`` - input layout, backbone with
BatchNorm folded, pools, lifter, fusion iterations, gaze heads - so its four outputs are bit-identical to the module's.
What depends on the weights only (sp weight copies, BatchNorm folds, index tables) is queued once by ``bind`` /
``refresh``; ``run`` queues the per-input launches, allocates nothing when given its outputs and never synchronises.

Two compute forms: the fp32 model (default), and with ``compute=torch.bfloat16`` the bf16 inference form - what ``run_views``
queues with ``compute_dtype = torch.bfloat16`` (BatchNorm folded into ``mvg_conv_fprop_bf16_affine``, uint8 patches straight
to the bf16 stem input, the Linears "mixed" on the bf16 matrix cores), again bit for bit.

The model's own ``forward`` / ``forward_multiview`` do not route through a session.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import torch

from . import ops
from ._lib import SESSION_BF16, SESSION_FP32, SessionCfg, check, lib
from .arch import NUM_FEAT_VEC, RANGE_OVER_BITS
from .heads import directed_pairs

Tensor = torch.Tensor


class InferenceSession:
    """``InferenceSession(model, views, batch, height, width, raw_hw=None, input_bgr=False, range_record=False, compute=None,
    meter=None)``.

    model: a ``MultiViewGaze`` / ``FeatRotationSymm`` on the GPU (default, ``share_weights`` or ``ignore_rotmat`` variant).
    compute: None - the fp32 form, ``model.compute_dtype`` must be float32; ``torch.bfloat16`` - the bf16 inference form,
    ``model.compute_dtype`` must be bfloat16 (the kernel-family switch below does not apply, and there are no range units:
    ``range_record=True`` gives empty reports).  height / width: the network's input size.  raw_hw = (h, w): the views are raw uint8
    ``[B, h, w, 3]`` patches, resized and normalised on the GPU (``input_bgr``: swap B and R first); otherwise fp32
    ``[B, 3, height, width]``.  The kernel family follows ``model._backbone.split`` (MVG_SPLIT); the 2 GiB guard of the split
    path is evaluated from the real sizes.  Several sessions may share one model.

    range_record=True: every forward also leaves the activation range record of the backbone's sp tensors (one word per name in
    ``range_unit_names``; same launches, same outputs, still no synchronisation) for ``range_report()`` / ``overflowed()``.  A
    session has no fallback: on an overflow build one over a model with ``_backbone.split = False``.

    meter: a ``metrics.AngularErrorMeter(num_iter, views * (views - 1), ...)``: every ``run(..., gt=labels)`` also adds the forward's
    gaze errors to the meter's device record (``mvg_session_set_error_record``: one more launch after the plan's last step, same
    four outputs, still no synchronisation).  The session owns the static label buffer the hook reads."""

    def __init__(self, model, views: int, batch: int, height: int, width: int, raw_hw: Optional[Tuple[int, int]] = None,
                 input_bgr: bool = False, range_record: bool = False, compute: Optional[torch.dtype] = None, meter=None) -> None:
        v = model._variant
        if v.encode_rotmat or v.share_feature:
            raise ValueError("InferenceSession: the encode_rotmat and share_feature variants are not served by the native session")
        if compute not in (None, torch.float32, torch.bfloat16):
            raise ValueError("InferenceSession: compute must be None, torch.float32 or torch.bfloat16")
        want = torch.bfloat16 if compute == torch.bfloat16 else torch.float32
        if model.compute_dtype != want:
            raise ValueError(f"InferenceSession: this session computes in {want} and model.compute_dtype is {model.compute_dtype}: "
                             "pass compute=torch.bfloat16 for a model on the bf16 path (compute=None serves the fp32 model)")
        self.compute = want
        self._h = None
        self.model = model
        model.ensure_layout()
        self.views, self.batch, self.height, self.width = int(views), int(batch), int(height), int(width)
        self.raw_hw = tuple(raw_hw) if raw_hw is not None else None
        in_h, in_w = self.raw_hw if self.raw_hw is not None else (0, 0)
        cfg = SessionCfg(depth=model._depth, num_iter=model._num_iter, views=self.views, batch=self.batch, height=self.height,
                         width=self.width, share_weights=int(v.share_weights), ignore_rotmat=int(v.ignore_rotmat),
                         split=int(model._backbone.split), raw_u8=int(self.raw_hw is not None), in_h=int(in_h), in_w=int(in_w),
                         input_bgr=int(bool(input_bgr)))
        h = C.c_void_p()
        check(lib().mvg_session_create_ex(C.byref(cfg), SESSION_BF16 if want == torch.bfloat16 else SESSION_FP32, C.byref(h)),
              "session_create")
        self._h = h
        self.tensor_names: List[str] = [lib().mvg_session_tensor_name(h, i).decode() for i in range(lib().mvg_session_num_tensors(h))]
        self.workspace_bytes = int(lib().mvg_session_workspace_bytes(h))
        self.launches = int(lib().mvg_session_launches(h))
        self.device = next(model.parameters()).device
        self.fc_dim, self.num_iter, self.dirs = model._fc_dim, model._num_iter, self.views * (self.views - 1)
        with torch.cuda.device(self.device):
            self._workspace = torch.empty(self.workspace_bytes, dtype=torch.uint8, device=self.device)
        self._views_arr = (C.c_void_p * self.views)()
        self.range_unit_names: List[str] = [lib().mvg_session_range_unit_name(h, i).decode()
                                            for i in range(lib().mvg_session_num_range_units(h))]
        self._range_record: Optional[Tensor] = None
        if range_record and self.range_unit_names:
            with torch.cuda.device(self.device):
                self._range_record = torch.zeros(len(self.range_unit_names), dtype=torch.int32, device=self.device)
            check(lib().mvg_session_set_range_record(h, C.c_void_p(self._range_record.data_ptr())), "session_set_range_record")
        self.meter = None
        self._gt: Optional[Tensor] = None
        self.consensus = None                       # bind_consensus: the static consensus outputs, or None
        self._cons_weights: Optional[Tensor] = None
        if meter is not None:
            self.bind_meter(meter)
        self.refresh()

    # ---------------------------------------------------------------- gaze error meter
    def bind_meter(self, meter) -> None:
        """Attach ``meter`` (None: detach - the plain forward again).  Host only: the library stores four pointers."""
        if self._h is None:
            raise RuntimeError("InferenceSession is closed")
        if meter is None:
            check(lib().mvg_session_set_error_record(self._h, None, None, None, 0), "session_set_error_record")
            self.meter = None
        else:
            if (meter.num_iter, meter.dirs) != (self.num_iter, self.dirs):
                raise ValueError(f"InferenceSession: the meter holds {meter.num_iter} x {meter.dirs} cells, the session's forward has "
                                 f"{self.num_iter} iterations x {self.dirs} directions")
            meter._ensure(self.device)
            if self._gt is None:
                with torch.cuda.device(self.device):
                    self._gt = torch.zeros(self.dirs, self.batch, 2, dtype=torch.float32, device=self.device)
            check(lib().mvg_session_set_error_record(self._h, C.c_void_p(self._gt.data_ptr()), C.c_void_p(meter.record.data_ptr()),
                                                     C.c_void_p(meter.err_out.data_ptr()) if meter.err_out is not None else None,
                                                     meter.capacity), "session_set_error_record")
            self.meter = meter
        self.launches = int(lib().mvg_session_launches(self._h))

    # ---------------------------------------------------------------- consensus gaze
    def bind_consensus(self, weights: Optional[Tensor] = None, stats: bool = False, enable: bool = True) -> None:
        """Every ``run`` also leaves the consensus gaze of its own ``preds`` and ``rot`` (``mvg_session_set_consensus``: one more
        launch after the plan's last step, same four outputs, still no synchronisation) in ``session.consensus``: static tensors
        ``{"head" [I,B,3], "views" [I,V,B,2]}`` and with ``stats=True`` ``"stats"`` [I,B,2] (resultant length, mean disagreement
        in degrees).  weights: a static fp32 ``[B,V]`` device tensor the caller refills before each ``run`` (None: all views count
        1).  ``enable=False`` (or ``unbind_consensus()``) detaches: the plain forward again.  Host only: the library stores four
        pointers."""
        if self._h is None:
            raise RuntimeError("InferenceSession is closed")
        if not enable:
            check(lib().mvg_session_set_consensus(self._h, None, None, None, None), "session_set_consensus")
            self.consensus, self._cons_weights = None, None
        else:
            I, V, B = self.num_iter, self.views, self.batch
            if weights is not None and (tuple(weights.shape) != (B, V) or weights.dtype != torch.float32 or weights.device != self.device
                                        or not weights.is_contiguous()):
                raise ValueError(f"InferenceSession.bind_consensus: weights must be a contiguous fp32 tensor of shape {(B, V)} on {self.device}")
            with torch.cuda.device(self.device):
                mk = lambda *s: torch.empty(*s, dtype=torch.float32, device=self.device)
                cons = {"head": mk(I, B, 3), "views": mk(I, V, B, 2)}
                if stats:
                    cons["stats"] = mk(I, B, 2)
            check(lib().mvg_session_set_consensus(self._h, C.c_void_p(weights.data_ptr()) if weights is not None else None,
                                                  C.c_void_p(cons["head"].data_ptr()), C.c_void_p(cons["views"].data_ptr()),
                                                  C.c_void_p(cons["stats"].data_ptr()) if stats else None), "session_set_consensus")
            self.consensus, self._cons_weights = cons, weights
        self.launches = int(lib().mvg_session_launches(self._h))

    def unbind_consensus(self) -> None:
        self.bind_consensus(enable=False)

    # ---------------------------------------------------------------- weights
    def refresh(self) -> None:
        """(Re)bind the model's parameters and BatchNorm buffers and queue the once-per-weights work on the current stream.
        Call it after the weights changed (an optimizer step, ``load_state_dict``, a write to the arena)."""
        if self._h is None:
            raise RuntimeError("InferenceSession is closed")
        self.model.ensure_layout()
        named = self.model._named_tensors()
        ptrs = (C.c_void_p * len(self.tensor_names))()
        for i, name in enumerate(self.tensor_names):
            t = named[name].detach()
            if t.dtype != torch.float32 or t.device != self.device:
                raise RuntimeError(f"InferenceSession: {name} must be an fp32 tensor on {self.device}")
            if t.numel() != lib().mvg_session_tensor_numel(self._h, i):
                raise RuntimeError(f"InferenceSession: {name} has {t.numel()} elements, the session expects "
                                   f"{lib().mvg_session_tensor_numel(self._h, i)}")
            if not (t.is_contiguous(memory_format=torch.channels_last) if (t.dim() == 4 and t.shape[2] > 1) else
                    (t.is_contiguous() or t.is_contiguous(memory_format=torch.channels_last))):
                raise RuntimeError(f"InferenceSession: {name} must be contiguous (conv weights channels_last = KRSC)")
            ptrs[i] = t.data_ptr()
        with torch.cuda.device(self.device):
            check(lib().mvg_session_bind(self._h, ptrs, C.c_void_p(self._workspace.data_ptr()), self.workspace_bytes,
                                         C.c_void_p(ops._s())), "session_bind")

    # ---------------------------------------------------------------- forward
    def empty_outputs(self):
        """Uninitialised (img_feat, lifted, feats, preds) of this session's shape, for ``run(..., out=...)``."""
        V, B, I, D, dev = self.views, self.batch, self.num_iter, self.dirs, self.device
        mk = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        return mk(V, B, self.fc_dim), mk(V, B, 3, NUM_FEAT_VEC), mk(I, D, B, 3, NUM_FEAT_VEC), mk(I, D, B, 2)

    def run(self, imgs: Sequence[Tensor], rot: Tensor, out=None, gt: Optional[Tensor] = None):
        """imgs: V tensors (fp32 ``[B,3,H,W]``, or uint8 ``[B,h,w,3]`` with ``raw_hw``); rot fp32 ``[B,V,3,3]``.  Returns
        ``(img_feat [V,B,Cf], lifted [V,B,3,512], feats [I,D,B,3,512], preds [I,D,B,2])`` as ``run_views`` does; ``out``
        (from ``empty_outputs``) receives them without any allocation.  Queued on the current stream.  gt ``[B,V,2]``: with a meter,
        the labels of this batch, copied (stream-ordered, one small copy per direction) into the session's static label buffer."""
        if self._h is None:
            raise RuntimeError("InferenceSession is closed")
        V, B = self.views, self.batch
        if len(imgs) != V:
            raise ValueError(f"InferenceSession.run: {len(imgs)} views, the session was made for {V}")
        want = (B, self.raw_hw[0], self.raw_hw[1], 3) if self.raw_hw is not None else (B, 3, self.height, self.width)
        dt = torch.uint8 if self.raw_hw is not None else torch.float32
        for v, im in enumerate(imgs):
            if tuple(im.shape) != want or im.dtype != dt or im.device != self.device or not im.is_contiguous():
                raise ValueError(f"InferenceSession.run: view {v} must be a contiguous {dt} tensor of shape {want} on {self.device}")
            self._views_arr[v] = im.data_ptr()
        if tuple(rot.shape) != (B, V, 3, 3) or rot.dtype != torch.float32 or rot.device != self.device or not rot.is_contiguous():
            raise ValueError(f"InferenceSession.run: rot must be a contiguous fp32 tensor of shape {(B, V, 3, 3)} on {self.device}")
        if out is None:
            out = self.empty_outputs()
        else:
            for o, ref in zip(out, ((V, B, self.fc_dim), (V, B, 3, NUM_FEAT_VEC), (self.num_iter, self.dirs, B, 3, NUM_FEAT_VEC),
                                    (self.num_iter, self.dirs, B, 2))):
                if tuple(o.shape) != ref or o.dtype != torch.float32 or o.device != self.device or not o.is_contiguous():
                    raise ValueError(f"InferenceSession.run: an output must be a contiguous fp32 tensor of shape {ref}")
        img_feat, lifted, feats, preds = out
        if (gt is None) != (self.meter is None):
            raise ValueError("InferenceSession.run: gt goes with a meter (a session with a meter needs every batch's labels)")
        if gt is not None:
            if tuple(gt.shape) != (B, V, 2) or gt.device != self.device:
                raise ValueError(f"InferenceSession.run: gt must have shape {(B, V, 2)} on {self.device}")
            for d, v in enumerate(directed_pairs(V)[0]):       # slices (metrics.build_gt_dir): a list index would synchronise
                self._gt[d].copy_(gt[:, v])
        with torch.cuda.device(self.device):
            check(lib().mvg_session_forward(self._h, self._views_arr, C.c_void_p(rot.data_ptr()), C.c_void_p(img_feat.data_ptr()),
                                            C.c_void_p(lifted.data_ptr()), C.c_void_p(feats.data_ptr()), C.c_void_p(preds.data_ptr()),
                                            C.c_void_p(ops._s())), "session_forward")
        return img_feat, lifted, feats, preds

    # ---------------------------------------------------------------- activation range record
    def range_report(self):
        """{conv name: max |activation| of the sp tensor its unit stored} in the last forward, in forward order; empty when the
        backbone is not on the split kernels.  Needs ``range_record=True``.  Synchronises."""
        if self._range_record is None:
            if self.range_unit_names:
                raise RuntimeError("InferenceSession: made without range_record=True")
            return {}
        vals = self._range_record.cpu().view(torch.float32).tolist()
        return dict(zip(self.range_unit_names, vals))

    def overflowed(self) -> List[str]:
        """The units of ``range_report()`` whose tensor reached 65 520 (an fp16 piece became inf), in forward order.  Synchronises."""
        if self._range_record is None:
            if self.range_unit_names:
                raise RuntimeError("InferenceSession: made without range_record=True")
            return []
        return [n for n, w in zip(self.range_unit_names, self._range_record.tolist()) if w >= RANGE_OVER_BITS]

    # ---------------------------------------------------------------- lifetime
    def close(self) -> None:
        """Destroy the handle and drop the workspace (stream-ordered: queued forwards still finish)."""
        if self._h is not None:
            lib().mvg_session_destroy(self._h)
            self._h = None
            self._workspace = None
            self._range_record = None
            self.meter = self._gt = None
            self.consensus = self._cons_weights = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
