"""Lifter + cross-view fusion + gaze heads, forward and backward, on the HIP kernels - generalised
from the reference's two views to V views (every unordered pair runs the reference's two-view
recurrence) and covering the constructor variants of the reference model.

What it replaces (for V = 2 exactly):
  * Feat3dLifter.forward ............ /root/reference/models/rot_mv.py:91-98
  * rot_10 / rot_01 .................. :193-194
  * the fusion loop .................. :205-263 with, per variant,
      default        ImageFeatFuser on rot @ F_partner ............ :35-50, :234-239
      ignore_rotmat  ImageFeatFuser on F_partner ................... :226-232
      encode_rotmat  ImageRotmatFeatFuser(img, F_partner, rot) ..... :53-69, :219-225
      share_feature  RotFeatFuser + IntensityBatchNorm on the lifted features :13-32, :72-86, :199-201, :241-247
      share_weights  one fuser / head reused by every iteration .... :148-156

Row space: D = V(V-1) *directed* pairs d = 2p (i<-j), 2p+1 (j<-i) for the p-th unordered pair
(i<j) in lexicographic order; every GEMM of an iteration runs over all D*B rows at once because
the two directions (and all pairs) share the iteration's weights.

One call, one record (as in backbone.py): plan_head decides on the host, from shapes and knobs alone, which kernel family
the fuser / head Linears of a forward call run on (HeadCall); layer_launch is the single per-layer rule every caller asks;
the record travels down as an argument and stays on the tape, where backward reads it.  Nothing of a call lives on the
FusionHead or its _Mlp modules - only caches that outlast calls do (index tables, the weight-copy buffers and their
versions)."""
from __future__ import annotations

import enum
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

from . import ops
from .arch import DEFAULT_VARIANT, NUM_FEAT_VEC, ROT_DIM, Variant
from .backbone import Family, GradSink

Tensor = torch.Tensor
IBN_MOMENTUM, IBN_EPS = 0.05, 1e-4          # IntensityBatchNorm defaults, rot_mv.py:14
SPLIT_MIN_ROWS = 1024                       # Linears with at least this many rows run on the split-operand kernels
SLOTS = 64                                  # floats in the split path's scale / abs-max arena (one per call, on its tape)


def directed_pairs(views: int) -> Tuple[List[int], List[int]]:
    vi, vj = [], []
    for i in range(views):
        for j in range(i + 1, views):
            vi += [i, j]
            vj += [j, i]
    return vi, vj


def _pad4(n: int) -> int:
    return (n + 3) // 4 * 4


def split_serves(num_iter: int) -> bool:
    """_forward_split names 11 scale slots per iteration plus 2 in its SLOTS-float arena and hands 2 + I tensors to one
    mvg_absmax_multi launch (at most 8): num_iter <= 5.  (csrc/session_plan.cpp: Builder::build holds the same limit.)"""
    return 2 + num_iter <= 8 and 11 * num_iter + 2 <= SLOTS


# ---------------------------------------------------------------- the plan of one call
class MlpShape(NamedTuple):
    """The Linear shapes of one [Linear + ReLU] * (n - 1), Linear stack.  Feature widths that are not multiples of 4
    (encode_rotmat: K_in + 9 = 2057 / 3593) run zero-padded (fin_p, fout_p): the GEMM kernels move 16-byte vectors along K.
    A last layer of at most 4 outputs (the heads' 512 -> 2) keeps its width: the skinny kernels serve it."""
    fin: Tuple[int, ...]
    fout: Tuple[int, ...]
    fin_p: Tuple[int, ...]
    fout_p: Tuple[int, ...]
    padded: Tuple[bool, ...]

    @classmethod
    def of(cls, layers) -> "MlpShape":
        """layers: (in_features, out_features) per Linear."""
        fin, fout = tuple(i for i, _ in layers), tuple(o for _, o in layers)
        n = len(fin)
        fin_p = tuple(_pad4(f) for f in fin)
        fout_p = tuple(f if (l == n - 1 and f <= 4) else _pad4(f) for l, f in enumerate(fout))
        return cls(fin, fout, fin_p, fout_p, tuple(fin_p[l] != fin[l] or fout_p[l] != fout[l] for l in range(n)))

    @property
    def n(self) -> int:
        return len(self.fin)

    def skinny(self, l: int) -> bool:
        return l == self.n - 1 and self.fout[l] <= 4

    def split_eligible(self, l: int) -> bool:
        """The split Linear kernels move whole 32-wide spans along both widths."""
        return not self.padded[l] and self.fin[l] % 32 == 0 and self.fout[l] % 32 == 0


class HeadCall(NamedTuple):
    """One FusionHead.forward call: what plan_head decided, plus this call's weight copies (wprep), which forward() makes.
    Passed down explicitly and kept on the tape; nothing of it lives on the FusionHead or its modules."""
    V: int
    B: int
    D: int                      # V (V - 1) directed pairs
    rows: int                   # D * B rows of every fuser / head GEMM
    I: int
    training: bool
    keep_tape: bool
    family: Family              # of the fuser and head Linears (the lifter, V * B rows: BF16 on a BF16 call, else FP32)
    fused_in: bool              # the first Linear of every fuser / head forms its input rows in its operand loader
    reuse_copies: bool          # BF16: the persistent bf16 copies may serve this call if the weights are unchanged
    wprep: Optional[Dict[tuple, tuple]] = None      # (module, layer) -> this call's (w, w_t) copies (SPLIT: sp, BF16: bf16)

    @property
    def mode(self) -> str:
        return {Family.FP32: "fp32", Family.SPLIT: "split", Family.BF16: "mixed"}[self.family]


def plan_head(variant: Variant, *, V: int, B: int, num_iter: int, cf: int, fuser: MlpShape, head: MlpShape, keep_tape: bool,
              training: bool, split: bool = True, mixed: bool = False, fused_input: bool = True,
              keep_infer_copies: bool = True) -> HeadCall:
    """The decisions of one forward call, from shapes and flags alone (no tensor, no device).  fuser / head: the Linear
    shapes of one fuser and one gaze head; split, mixed, fused_input, keep_infer_copies: the FusionHead attributes of the
    same names.

    BF16 (mixed) wins.  SPLIT needs the default or ignore_rotmat form of the inputs (the other variants have 9 extra
    columns / interleaved rows), at least SPLIT_MIN_ROWS rows, an iteration count the slot arena serves (split_serves) and
    the three Linears _forward_split drives - both fuser layers and the head's first - split-eligible; else the call runs
    on the fp32 Linears.  (With ResNet-18 / -50 those three are 2048 or 3584 wide: the last condition always holds.)
    fused_in: default / ignore_rotmat variants on the fp32 Linears - rotate + concat run inside the first Linear's operand
    loader; the split Linears' span loader and the bf16 Linears read plain, materialised rows."""
    D = V * (V - 1)
    rows = D * B
    plain = not (variant.share_feature or variant.encode_rotmat)
    if mixed:
        family = Family.BF16
    elif (split and plain and rows >= SPLIT_MIN_ROWS and split_serves(num_iter) and fuser.n == 2
          and fuser.split_eligible(0) and fuser.split_eligible(1) and head.split_eligible(0)):
        family = Family.SPLIT
    else:
        family = Family.FP32
    fused_in = fused_input and plain and family is Family.FP32
    assert not fused_in or (fuser.fin[0] == head.fin[0] == cf + 3 * NUM_FEAT_VEC and not fuser.padded[0] and not head.padded[0])
    return HeadCall(V, B, D, rows, num_iter, training, keep_tape, family, fused_in,
                    reuse_copies=keep_infer_copies and not keep_tape and not training)


class Launch(enum.Enum):
    """The launch a Linear layer runs (layer_launch)."""
    GEN = 0       # fp32, input rows formed in the operand loader (mvg_fuser_fprop / mvg_fuser_wgrad)
    FP32 = 1      # fp32-MFMA on the parameters themselves
    PADDED = 2    # fp32-MFMA on zero-padded copies of the parameters
    SKINNY = 3    # at most 4 outputs (mvg_linear_skinny_fwd / _bwd)
    BF16 = 4      # fp32 tensors, products on the bf16 cores against bf16 weight copies ("mixed")
    SPLIT = 5     # split-operand kernels, operands in sp (driven by _forward_split / _backward_split)


def layer_launch(call: HeadCall, s: MlpShape, l: int, lifter: bool = False) -> Launch:
    """The launch that runs layer ``l`` of a stack of shape ``s`` in ``call``.  Padded and skinny layers stay fp32 whatever
    the family; the lifter follows the call only to BF16."""
    assert not (s.padded[l] and s.skinny(l))
    if s.padded[l]:
        return Launch.PADDED
    if s.skinny(l):
        return Launch.SKINNY
    if call.family is Family.BF16:
        return Launch.BF16
    if lifter:
        return Launch.FP32
    if call.family is Family.SPLIT and s.split_eligible(l):
        return Launch.SPLIT
    return Launch.GEN if (l == 0 and call.fused_in) else Launch.FP32


class _Written:
    """Parameters whose gradient this backward has already written: a second write (weights shared
    between iterations) must accumulate whatever ``sink.accumulate`` said at the start."""

    def __init__(self, sink: GradSink, side=None):
        self.sink = sink
        self.seen = set()
        self.side = side          # low-priority stream for the weight / bias gradients (off the critical path)

    def off_path(self, fn, *tensors):
        """Run fn (kernels that only produce parameter gradients) on the side stream, after everything
        queued so far; `tensors` are its inputs (kept from the allocator until the side stream is done)."""
        if self.side is None:
            fn()
            return
        self.side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.side):
            fn()
        for t in tensors:
            t.record_stream(self.side)

    def acc(self, p) -> bool:
        a = self.sink.accumulate(p) or id(p) in self.seen
        self.seen.add(id(p))
        return a


class _GenInput:
    """Rows [ img_feat[row_img[m]] | rel[m] @ feat[row_src[m]] ] of a fuser / head input, described instead of
    stored: the first Linear's kernels build them in their operand loaders (ops.fuser_fprop / fuser_wgrad)."""
    __slots__ = ("img", "feat", "rel", "row_img", "row_src", "cf", "nvec", "rows", "width")

    def __init__(self, img, feat, rel, row_img, row_src, cf, nvec):
        self.img, self.feat, self.rel, self.row_img, self.row_src, self.cf, self.nvec = img, feat, rel, row_img, row_src, cf, nvec
        self.rows, self.width = row_img.shape[0], cf + 3 * nvec


class _Slots:
    """The split path's arena: SLOTS floats (abs-max values and the scales made from them) named on first use.  The tape
    keeps the tensor and the name -> index map; backward names further slots in the same arena."""

    def __init__(self, st: Tensor, names: Dict[str, int]):
        self.st, self.names = st, names

    def slot(self, name: str) -> Tensor:
        i = self.names.setdefault(name, len(self.names))
        return self.st[i:i + 1]

    def sp(self, r: int, c: int, name: str) -> Tensor:
        """An empty [r, c] sp tensor whose 2^-k is the slot ``name``."""
        t = ops.sp_empty(r, c, device=self.st.device)
        t.sinv = self.slot(name)
        return t


class _Saved(NamedTuple):
    """What one iteration of the fp32 / bf16 forward keeps: the fuser and head inputs (a _GenInput where they were never
    written), the hidden activations (one per hidden layer) and the IntensityBatchNorm scales (share_feature)."""
    x: object
    hf: List[Tensor]
    xh: object
    hh: List[Tensor]
    scales: Optional[Tensor]


class _SavedSplit(NamedTuple):
    """What one iteration of _forward_split keeps: the fuser input and hidden activation (sp), the head input (sp) and
    hidden activation (fp32), and the (w, w_t) sp copies of the three split Linears."""
    xf: Tensor
    h: Tensor
    xh: Tensor
    hh: Tensor
    wf0: tuple
    wf1: tuple
    wh0: tuple


class _Mlp:
    """[Linear + ReLU] * (n - 1), Linear  (/root/reference/models/backbones/blocks.py:27-60; two layers
    for the lifter, ImageFeatFuser and the heads, three for ImageRotmatFeatFuser / RotFeatFuser).

    Padded layers (MlpShape) run on zero-padded copies of the weights, refreshed from the parameters every forward;
    padded hidden units are relu(0) = 0.  forward / backward are the fp32-MFMA and bf16-mixed launches of a call
    (layer_launch); the split Linears are driven by FusionHead._forward_split / _backward_split."""

    def __init__(self, params: Dict[str, Tensor], prefix: str, n_layers: int = 2, lifter: bool = False):
        self.w = [params[f"{prefix}blocks.{l}.0.weight"] for l in range(n_layers)]
        self.b = [params[f"{prefix}blocks.{l}.0.bias"] for l in range(n_layers)]
        self.n, self.lifter = n_layers, lifter
        self.shape = MlpShape.of([(w.shape[1], w.shape[0]) for w in self.w])
        self.fin, self.fout, self.fin_p, self.fout_p, self.padded = self.shape
        self._wp: List[Optional[Tensor]] = [None] * n_layers
        self._bp: List[Optional[Tensor]] = [None] * n_layers
        self.in_width = self.fin_p[0]

    def launch(self, call: HeadCall, l: int) -> Launch:
        return layer_launch(call, self.shape, l, self.lifter)

    def parameters(self):
        out = []
        for w, b in zip(self.w, self.b):
            out += [w, b]
        return out

    def _weights(self, l: int):
        if not self.padded[l]:
            return self.w[l].detach(), self.b[l].detach()
        if self._wp[l] is None or self._wp[l].device != self.w[l].device:
            self._wp[l] = torch.zeros(self.fout_p[l], self.fin_p[l], dtype=torch.float32, device=self.w[l].device)
            self._bp[l] = torch.zeros(self.fout_p[l], dtype=torch.float32, device=self.w[l].device)
        self._wp[l][: self.fout[l], : self.fin[l]].copy_(self.w[l].detach())       # layout plumbing
        self._bp[l][: self.fout[l]].copy_(self.b[l].detach())
        return self._wp[l], self._bp[l]

    def forward(self, call: HeadCall, x: Optional[Tensor], out: Optional[Tensor] = None, gen: Optional[_GenInput] = None):
        """x [rows, in_width] -> (hidden activations [h_0 .. h_{n-2}], y [rows, fout_last]).
        gen (instead of x, where layer 0 is Launch.GEN): the input rows [img_feat | R @ F] are generated inside the first
        layer's GEMM (mvg_fuser_fprop) - the concatenated / rotated operand is never materialised."""
        if gen is not None:
            assert x is None and self.launch(call, 0) is Launch.GEN and gen.width == self.fin_p[0]
            rows, dev = gen.rows, gen.img.device
        else:
            rows, dev = x.shape[0], x.device
            assert x.shape[1] == self.fin_p[0], (x.shape, self.fin_p[0])
        hs: List[Tensor] = []
        cur = x
        for l in range(self.n):
            w, b = self._weights(l)
            last = l == self.n - 1
            kind = self.launch(call, l)
            y = out if (last and out is not None) else torch.empty(rows, self.fout_p[l], dtype=torch.float32, device=dev)
            if kind is Launch.BF16:
                ops.linear_fprop_mixed(cur, call.wprep[self, l][0], b, not last, y, rows, self.fin_p[l], self.fout_p[l])
            elif kind is Launch.GEN:
                ops.fuser_fprop(gen.img, gen.feat, gen.rel, gen.row_img, gen.row_src, w, b, not last, y, rows, gen.cf, gen.nvec,
                                self.fout_p[l])
            elif kind is Launch.SKINNY:
                ops.linear_skinny_fwd(cur, w, b, y, rows, self.fin_p[l], self.fout[l])
            else:
                assert kind in (Launch.FP32, Launch.PADDED), kind
                ops.linear_fprop(cur, w, b, not last, y, rows, self.fin_p[l], self.fout_p[l])
            if not last:
                hs.append(y)
            cur = y
        return hs, cur

    def backward(self, call: HeadCall, x: Optional[Tensor], hs: List[Tensor], gy: Tensor, sink: GradSink, wr: _Written,
                 dx_addend: Optional[Tensor] = None, dx_out: Optional[Tensor] = None, gen: Optional[_GenInput] = None) -> Tensor:
        """gy = grad wrt the output; returns grad wrt x (optionally fused `+ dx_addend`).  gen: see forward
        (the first layer's weight gradient regenerates the input rows inside mvg_fuser_wgrad)."""
        rows, dev = gy.shape[0], gy.device
        g = gy
        for l in range(self.n - 1, -1, -1):
            inp = x if l == 0 else hs[l - 1]
            kind = self.launch(call, l)
            w, _ = self._weights(l) if kind is Launch.PADDED else (self.w[l].detach(), None)
            fin, fout = self.fin_p[l], self.fout_p[l]
            # ---- weight / bias gradients
            if kind is Launch.PADDED:
                accs = (wr.acc(self.w[l]), wr.acc(self.b[l]))

                def padded_grads(inp=inp, g=g, l=l, fin=fin, fout=fout, accs=accs):
                    dwp = torch.empty(fout, fin, dtype=torch.float32, device=dev)
                    dbp = torch.empty(fout, dtype=torch.float32, device=dev)
                    ops.linear_wgrad(inp, g, dwp, dbp, rows, fin, fout, False)
                    for p, src, a in ((self.w[l], dwp[: self.fout[l], : self.fin[l]], accs[0]),
                                      (self.b[l], dbp[: self.fout[l]], accs[1])):
                        if a:
                            sink.view(p).add_(src)
                        else:
                            sink.view(p).copy_(src)
                wr.off_path(padded_grads, inp, g)
            elif kind is Launch.SKINNY:
                aw, ab = wr.acc(self.w[l]), wr.acc(self.b[l])
                assert aw == ab
                dh = torch.empty(rows, fin, dtype=torch.float32, device=dev)
                ops.linear_skinny_bwd(g, inp, w, inp, dh, sink.view(self.w[l]), sink.view(self.b[l]), rows, fin, self.fout[l], aw)
                g = dh                               # skinny_bwd already applied the ReLU mask of its input
                continue
            else:
                assert kind in (Launch.FP32, Launch.GEN, Launch.BF16), kind
                aw, ab = wr.acc(self.w[l]), wr.acc(self.b[l])
                assert aw == ab

                def grads(inp=inp, g=g, l=l, fin=fin, fout=fout, aw=aw, kind=kind):
                    # weight AND bias gradient in one launch: the bias gradient (column sums of g) rides on the
                    # kernel that streams g for the weight gradient
                    if kind is Launch.BF16:
                        ops.linear_wgrad_mixed(inp, g, sink.view(self.w[l]), sink.view(self.b[l]), rows, fin, fout, aw)
                    elif kind is Launch.GEN:
                        ops.fuser_wgrad(gen.img, gen.feat, gen.rel, gen.row_img, gen.row_src, g, sink.view(self.w[l]),
                                        sink.view(self.b[l]), rows, gen.cf, gen.nvec, fout, aw)
                    else:
                        ops.linear_wgrad(inp, g, sink.view(self.w[l]), sink.view(self.b[l]), rows, fin, fout, aw)
                if kind is Launch.GEN:
                    # every per-step tensor the side-stream kernel reads must be recorded on that stream: `rel` is
                    # a per-forward allocation owned only by this tape (the row tables are cached for the model's life)
                    wr.off_path(grads, gen.img, gen.feat, g, *([gen.rel] if gen.rel is not None else []))
                else:
                    wr.off_path(grads, inp, g)
            # ---- input gradient: (g @ W) [* (h > 0)] [+ dx_addend]
            dx = dx_out if (l == 0 and dx_out is not None) else torch.empty(rows, fin, dtype=torch.float32, device=dev)
            mask, addend = (None, dx_addend) if l == 0 else (hs[l - 1], None)
            if kind is Launch.BF16:
                ops.linear_dgrad_mixed(g, call.wprep[self, l][1], mask, addend, dx, rows, fin, fout)
            else:
                ops.linear_dgrad(g, w, mask, addend, dx, rows, fin, fout)
            g = dx
        return g


class FusionHead:
    _SLOTS = SLOTS
    split_serves = staticmethod(split_serves)

    def __init__(self, params: Dict[str, Tensor], fc_dim: int, num_iter: int, variant: Variant = DEFAULT_VARIANT):
        self.cf, self.I, self.v = fc_dim, num_iter, variant
        self.lifter = _Mlp(params, "_lifter._lifter.", 2, lifter=True)
        three = variant.encode_rotmat or variant.share_feature
        self.fusers = [_Mlp(params, f"_img_fusers.{i}._fuser.", 3 if three else 2) for i in range(num_iter)]
        self.heads = [_Mlp(params, f"_gaze_estimators.{i}.", 2) for i in range(num_iter)]
        if variant.share_weights:                     # nn.ModuleList([module] * num_iter): one module
            self.fusers = [self.fusers[0]] * num_iter
            self.heads = [self.heads[0]] * num_iter
        self.ibn = [params[f"_img_fusers.{i}._batchnorm.running_mean"] for i in range(num_iter)] \
            if variant.share_feature else None
        # The knobs of a call (plan_head reads them when forward is called; nothing else does):
        self.fused_input = True                   # MVG_FUSED_INPUT=0: materialise the fuser / head inputs with rotcat kernels instead (A/B switch)
        self.mixed = False                        # bf16 path: Linear products on the bf16 matrix cores (set by the model per call)
        self.split = True                         # fp32 path: Linears with >= SPLIT_MIN_ROWS rows on the split-operand kernels
        self.keep_infer_copies = True             # bf16 path: inference calls reuse the bf16 copies while the weights are unchanged
        self.kin = self.fusers[0].in_width            # row length of the fuser input (zero-padded)
        self.hin = self.heads[0].in_width
        # Caches across calls:
        self._idx_cache: Dict[Tuple[int, str], dict] = {}
        self._wprep_state = None                  # the persistent weight-copy buffers and their record table (_prepare_weights)
        self._wprep_versions = None               # the parameter versions those buffers hold (the tapes that point into them rely on it)
        self._wbf_infer_ok = False                # the persistent bf16 copies hold _wprep_versions and may serve the next inference call

    def invalidate_weight_cache(self):
        """The next inference call of the bf16 path casts the Linear weights again (see Backbone.invalidate_weight_cache)."""
        self._wbf_infer_ok = False

    def _prepare_weights(self, call: HeadCall, dev) -> Optional[Dict[tuple, tuple]]:
        """(module, layer) -> (w, w_t) for every Linear of ``call`` that runs on the split kernels (sp copies: KRSC for fprop,
        CRSK for backward-data) or on the bf16 kernels (bf16 copies), made by ONE batched launch pair (like
        Backbone._prepare_weights: persistent destination buffers and a device-resident record table built once per
        parameter placement).  None on a call that needs no copies."""
        if call.family is Family.FP32:
            return None
        mixed = call.family is Family.BF16
        mods = ([self.lifter] if mixed else []) + self.unique_modules()
        want = Launch.BF16 if mixed else Launch.SPLIT
        layers = [(m, l) for m in mods for l in range(m.n) if m.launch(call, l) is want]
        if not layers:
            return None
        key = (str(dev), mixed, tuple(m.w[l].data_ptr() for m, l in layers))
        if self._wprep_state is None or self._wprep_state[0] != key:
            wstat = torch.zeros(len(layers), 2, dtype=torch.float32, device=dev)
            rows_t, copies = [], {}
            for i, (m, l) in enumerate(layers):
                fin, fout = m.fin[l], m.fout[l]
                if mixed:
                    wk = torch.empty(fout, 1, 1, fin, dtype=torch.bfloat16, device=dev)
                    wt = torch.empty(fin, 1, 1, fout, dtype=torch.bfloat16, device=dev)
                else:
                    wk, wt = ops.sp_empty(fout, fin, device=dev), ops.sp_empty(fin, fout, device=dev)
                    wk.sinv = wt.sinv = wstat[i, 1:2]
                copies[m, l] = (wk, wt)
                rows_t.append([m.w[l].data_ptr(), wk.data_ptr(), wt.data_ptr(), fout | (1 << 32), fin | (fin << 32), wstat[i].data_ptr()])
            self._wprep_state = (key, copies, torch.tensor(rows_t, dtype=torch.int64).to(dev), wstat)
            self._wbf_infer_ok = False
        _, copies, table, wstat = self._wprep_state
        versions = tuple(m.w[l]._version for m, l in copies)
        # reuse (bf16 inference): the buffers already hold these parameters (same placement, same version counters, nothing
        # invalidated since) - no cast launch
        if mixed and call.reuse_copies and self._wbf_infer_ok and self._wprep_versions == versions:
            return copies
        self._wbf_infer_ok = mixed and call.reuse_copies
        if not mixed:
            wstat.zero_()
        ops.weights_prep_batch(table, len(copies), 0 if mixed else 1, 256)
        self._wprep_versions = versions
        return copies

    def unique_modules(self) -> List[_Mlp]:
        """Heads and fusers in grad-ready order (last iteration first), each module once."""
        out, seen = [], set()
        for it in range(self.I - 1, -1, -1):
            for m in (self.heads[it], self.fusers[it]):
                if id(m) not in seen:
                    seen.add(id(m))
                    out.append(m)
        return out

    def _indices(self, views: int, dev) -> dict:
        key = (views, str(dev))
        if key not in self._idx_cache:
            vi, vj = directed_pairs(views)
            D = len(vi)
            mk = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)
            self._idx_cache[key] = {"vi": mk(vi), "vj": mk(vj), "partner": mk([d ^ 1 for d in range(D)]),
                                    "ident": mk(list(range(D))), "D": D}
        return self._idx_cache[key]

    def _row_tables(self, views: int, batch: int, dev) -> dict:
        """Row-index tables (int32, device) of the generated fuser / head inputs: row (d, b) takes the image feature
        of view vi[d] and the source feature row given by the table (partner view / partner direction / itself)."""
        key = (views, batch, str(dev), "rows")
        if key not in self._idx_cache:
            vi, vj = directed_pairs(views)
            D = len(vi)
            b = torch.arange(batch, dtype=torch.int32)
            tab = lambda idx: (torch.tensor(idx, dtype=torch.int32)[:, None] * batch + b[None, :]).reshape(-1).contiguous().to(dev)
            self._idx_cache[key] = {"img": tab(vi), "view": tab(vj), "partner": tab([d ^ 1 for d in range(D)]),
                                    "ident": tab(list(range(D)))}
        return self._idx_cache[key]

    # ---------------------------------------------------------------- operand builders
    def _fuser_input(self, a: Tensor, src: Tensor, rel: Tensor, vi, src_idx, B: int, D: int, scales):
        """Rows (d, b) of the fuser's input.  a = image features [V,B,Cf] (lifted features [V,B,3,512]
        for share_feature); src = the partner features, addressed through src_idx."""
        dev, v = a.device, self.v
        X = torch.empty(D * B, self.kin, dtype=torch.float32, device=dev)
        if v.share_feature:
            ops.paircat_fwd(a, src, rel, scales, vi, src_idx, X, B, D, NUM_FEAT_VEC)
        elif v.encode_rotmat:
            ops.rotcat_ext_fwd(a, src, None, rel, vi, src_idx, X, self.kin, B, D, self.cf, NUM_FEAT_VEC)
        else:
            ops.rotcat_fwd(a, src, None if v.ignore_rotmat else rel, vi, src_idx, X, B, D, self.cf, NUM_FEAT_VEC)
        return X

    def _head_input(self, a: Tensor, feat: Tensor, vi, ident, B: int, D: int):
        Xh = torch.empty(D * B, self.hin, dtype=torch.float32, device=a.device)
        if self.v.share_feature:
            ops.paircat_fwd(a, feat, None, None, vi, ident, Xh, B, D, NUM_FEAT_VEC)
        else:
            ops.rotcat_fwd(a, feat, None, vi, ident, Xh, B, D, self.cf, NUM_FEAT_VEC)
        return Xh

    # ---------------------------------------------------------------- forward
    def forward(self, img_feat: Tensor, rot: Tensor, keep_tape: bool, training: bool = True):
        """img_feat [V,B,Cf]; rot [B,V,3,3].  Returns (lifted [V,B,3,512], feats [I,D,B,3,512],
        preds [I,D,B,2], tape).
        csrc/session_plan.cpp restates the inference launches of this method as data: plan_head's family rule and the
        launches of _forward_fp32 (fused_in) and _forward_split in build, those of _forward_fp32 on a BF16 call
        (materialised _fuser_input / _head_input, layer_launch per layer) in build_bf16.  A change to the rules or the
        launches here must be made there too."""
        V, B, cf = img_feat.shape
        dev = img_feat.device
        call = plan_head(self.v, V=V, B=B, num_iter=self.I, cf=cf, fuser=self.fusers[0].shape, head=self.heads[0].shape,
                         keep_tape=keep_tape, training=training, split=self.split, mixed=self.mixed, fused_input=self.fused_input,
                         keep_infer_copies=self.keep_infer_copies)
        call = call._replace(wprep=self._prepare_weights(call, dev))
        ix = self._indices(V, dev)
        D, I, NV = call.D, call.I, NUM_FEAT_VEC
        # what every call starts with: the lifter (V * B rows), the relative rotations, the output buffers
        hl, lifted = self.lifter.forward(call, img_feat.reshape(V * B, cf))
        rel = torch.empty(D, B, 3, 3, dtype=torch.float32, device=dev)
        ops.relative_rotation(rot.detach().to(torch.float32).contiguous(), ix["vi"], ix["vj"], rel, B, V, D)
        feats = torch.empty(I, D * B, ROT_DIM, dtype=torch.float32, device=dev)
        preds = torch.empty(I, D * B, 2, dtype=torch.float32, device=dev)
        tape = {"call": call, "mode": call.mode, "img_feat": img_feat, "lifted": lifted, "hl": hl, "rel": rel, "V": V, "B": B,
                "wprep_versions": self._wprep_versions if call.wprep is not None else None}
        if call.family is Family.SPLIT:
            slots = _Slots(torch.zeros(SLOTS, dtype=torch.float32, device=dev), {})      # abs-max slots must start at zero
            tape.update(st=slots.st, slots=slots.names)
            tape["saved"] = self._forward_split(call, img_feat, lifted, rel, feats, preds, slots)
        else:
            tape["saved"] = self._forward_fp32(call, img_feat, lifted, rel, feats, preds, training)
        return lifted.view(V, B, 3, NV), feats.view(I, D, B, 3, NV), preds.view(I, D, B, 2), tape if keep_tape else None

    def _forward_fp32(self, call: HeadCall, img_feat: Tensor, lifted: Tensor, rel: Tensor, feats: Tensor, preds: Tensor,
                      training: bool) -> List[_Saved]:
        """The iterations on the fp32-MFMA Linears (and, a BF16 call, the bf16-mixed ones): _Mlp.forward per fuser / head."""
        V, B, D, cf, NV = call.V, call.B, call.D, self.cf, NUM_FEAT_VEC
        dev = img_feat.device
        ix = self._indices(V, dev)
        a = lifted if self.v.share_feature else img_feat       # rot_mv.py:199-201
        saved = []
        src, src_idx = lifted, ix["vj"]                  # iteration 0 reads the partner VIEW's lifted feature
        # fused_in: the fuser input X = [img_feat | R @ F] and the head input [img_feat | F] are never written
        rt = self._row_tables(V, B, dev) if call.fused_in else None
        img2d = img_feat.reshape(V * B, cf)
        for it in range(call.I):
            scales = None
            if call.fused_in:
                X = _GenInput(img2d, src.reshape(-1, ROT_DIM), None if self.v.ignore_rotmat else rel, rt["img"],
                              rt["view"] if it == 0 else rt["partner"], cf, NV)
                Hf, Fn = self.fusers[it].forward(call, None, feats[it], gen=X)
                Xh = _GenInput(img2d, Fn, None, rt["img"], rt["ident"], cf, NV)
                Hh, _ = self.heads[it].forward(call, None, preds[it], gen=Xh)
            else:
                if self.v.share_feature:
                    scales = torch.empty(2 * D, NV, dtype=torch.float32, device=dev)
                    ops.ibn_scales(a, src, ix["vi"], src_idx, self.ibn[it], training, IBN_MOMENTUM, IBN_EPS, scales, B, D, NV)
                X = self._fuser_input(a, src, rel, ix["vi"], src_idx, B, D, scales)
                Hf, Fn = self.fusers[it].forward(call, X, feats[it])
                Xh = self._head_input(a, Fn, ix["vi"], ix["ident"], B, D)
                Hh, _ = self.heads[it].forward(call, Xh, preds[it])
            if call.keep_tape:
                saved.append(_Saved(X, Hf, Xh, Hh, scales))
            src, src_idx = Fn, ix["partner"]             # view j's feature of the SAME pair, previous iteration
        return saved

    # ---------------------------------------------------------------- the split-operand path (fp32 model, >= SPLIT_MIN_ROWS rows)
    def _forward_split(self, call: HeadCall, img_feat: Tensor, lifted: Tensor, rel: Tensor, feats: Tensor, preds: Tensor,
                       slots: _Slots) -> List[_SavedSplit]:
        """The fuser / head Linears on the split kernels (conv_split.hip), every operand with its own power-of-two scale.

        Per iteration: fuser L1 (hidden activation written in sp, scaled from a bound), fuser L2 (fp32 features + their
        abs-max from the epilogue), ONE builder launch that writes this iteration's head input and the next iteration's
        fuser input straight into sp (mvg_fuse_build_split), head L1, head L2 (512 -> 2).  No fp32 copy of an operand is
        ever made and no separate abs-max / split pass runs: the scales come from device slots that the producing launches
        fill (the SLOTS-float arena owned by this call's tape)."""
        V, B, I, rows, cf, NV, kin = call.V, call.B, call.I, call.rows, self.cf, NUM_FEAT_VEC, self.kin
        dev = img_feat.device
        if not split_serves(I):                      # (plan_head decides this before forward comes here)
            raise RuntimeError(f"FusionHead: num_iter {I} is more than the split path's slot arena serves (at most 5)")
        slot, sp = slots.slot, slots.sp
        rel_fuse = None if self.v.ignore_rotmat else rel
        rt = self._row_tables(V, B, dev)
        img2d = img_feat.reshape(V * B, cf)
        ops.absmax_multi([img2d, lifted] + [self.fusers[it].b[0].detach() for it in range(I)],
                         [slot("am_img"), slot("am_lift")] + [slot(f"bam{it}") for it in range(I)])
        hh = torch.empty(I, rows, self.heads[0].fout[0], dtype=torch.float32, device=dev)
        xf = sp(rows, kin, "xf0")
        ops.fuse_build_split(img2d, lifted, rel_fuse, rt["img"], rt["view"], None, xf, None, slot("am_img"), slot("am_lift"), rows, cf, NV)
        saved = []
        for it in range(I):
            fu, hd = self.fusers[it], self.heads[it]
            assert fu.launch(call, 0) is fu.launch(call, 1) is hd.launch(call, 0) is Launch.SPLIT and hd.launch(call, 1) is Launch.SKINNY
            wf0, wf1, wh0 = call.wprep[fu, 0], call.wprep[fu, 1], call.wprep[hd, 0]
            hid, hhid = fu.fout[0], hd.fout[0]
            h = sp(rows, hid, f"h{it}")
            ops.linear_fprop_split(xf, wf0[0], fu.b[0].detach(), True, h, rows, kin, hid, bias_absmax=slot(f"bam{it}"))
            ops.linear_fprop_split(h, wf1[0], fu.b[1].detach(), False, feats[it], rows, hid, ROT_DIM, out_absmax=slot(f"amF{it}"))
            xh = sp(rows, kin, f"xh{it}")
            xf_next = sp(rows, kin, f"xf{it + 1}") if it + 1 < I else None
            ops.fuse_build_split(img2d, feats[it], rel_fuse, rt["img"], rt["partner"], rt["ident"], xf_next, xh, slot("am_img"),
                                 slot(f"amF{it}"), rows, cf, NV)
            ops.linear_fprop_split(xh, wh0[0], hd.b[0].detach(), True, hh[it], rows, kin, hhid)
            ops.linear_skinny_fwd(hh[it], hd.w[1].detach(), hd.b[1].detach(), preds[it], rows, hhid, 2)
            if call.keep_tape:
                saved.append(_SavedSplit(xf, h, xh, hh[it], wf0, wf1, wh0))
            xf = xf_next
        return saved

    def _backward_split(self, tape: dict, d_feats: Optional[Tensor], d_preds: Optional[Tensor], sink: GradSink, wr: _Written,
                        da: Tensor):
        """Backward of _forward_split, down to the gradient of the lifted features.  Per iteration, on the critical path:
        head L2 backward (its dx with the abs-max), [split + bias gradient -> head L1 dgrad], ONE mvg_fuse_unbuild (dF_it
        from the head input's and the next fuser input's gradients, the image-feature gradient sums), then for fuser L2
        and L1: split + bias gradient (one launch, scaled from the slot the producer filled) -> dgrad (with the next
        abs-max in its epilogue).  Weight gradients run on the side stream.  Returns (dlift or None, da_live)."""
        call: HeadCall = tape["call"]
        V, B, D, I, rows, cf, NV, kin, v = call.V, call.B, call.D, call.I, call.rows, self.cf, NUM_FEAT_VEC, self.kin, self.v
        rel, st = tape["rel"], tape["st"]
        dev = rel.device
        ix = self._indices(V, dev)
        slots = _Slots(st, tape["slots"])
        slot, sp = slots.slot, slots.sp
        rel_fuse = None if v.ignore_rotmat else rel
        da_live = False
        dXn: Optional[Tensor] = None                 # gradient of the NEXT iteration's fuser input

        def wgrad(x_sp, g_sp, p, fin, fout, acc):
            wr.off_path(lambda: ops.linear_wgrad_split(x_sp, g_sp, sink.view(p), rows, fin, fout, acc), x_sp, g_sp, st)

        for it in range(I - 1, -1, -1):
            xf, h, xh, hh, wf0, wf1, wh0 = tape["saved"][it]
            fu, hd = self.fusers[it], self.heads[it]
            hid, hhid = fu.fout[0], hd.fout[0]
            dXh = None
            if d_preds is not None:
                gp = d_preds[it].reshape(rows, 2).contiguous()
                a1, ab1 = wr.acc(hd.w[1]), wr.acc(hd.b[1])
                assert a1 == ab1
                dhh = torch.empty(rows, hhid, dtype=torch.float32, device=dev)
                ops.linear_skinny_bwd(gp, hh, hd.w[1].detach(), hh, dhh, sink.view(hd.w[1]), sink.view(hd.b[1]), rows, hhid, 2, a1,
                                      dx_absmax=slot(f"am_dhh{it}"))
                a0, ab0 = wr.acc(hd.w[0]), wr.acc(hd.b[0])
                assert a0 == ab0
                g_hh = sp(rows, hhid, f"g_hh{it}")
                ops.split_colsum(dhh, rows, hhid, slot(f"am_dhh{it}"), g_hh, sink.view(hd.b[0]), ab0)
                wgrad(xh, g_hh, hd.w[0], kin, hhid, a0)
                dXh = torch.empty(rows, kin, dtype=torch.float32, device=dev)
                ops.linear_dgrad_split(g_hh, wh0[1], dXh, rows, kin, hhid)
            else:
                self._zero_grads(hd, sink, wr)
            ext = d_feats[it].reshape(rows, ROT_DIM).contiguous() if d_feats is not None else None
            if dXh is None and dXn is None and ext is None:
                self._zero_grads(fu, sink, wr)
                if not v.share_weights:
                    sink.publish(hd.parameters() + fu.parameters())
                continue
            am_dF = slot(f"am_dF{it}")
            if dXh is None and dXn is None:
                dF = ext.clone()
            else:
                dF = torch.empty(rows, ROT_DIM, dtype=torch.float32, device=dev)
                ops.fuse_unbuild(dXh, dXn, rel_fuse, ix["partner"], ix["vi"], dF, da, da_live, D, V, D, B, cf, NV,
                                 absmax=am_dF if ext is None else None)
                da_live = True
                if ext is not None:
                    ops.axpby(ext, dF, 1.0, 1.0)
            if ext is not None:
                ops.absmax_multi([dF], [am_dF])
            # fuser layer 2: features <- hidden
            a1, ab1 = wr.acc(fu.w[1]), wr.acc(fu.b[1])
            assert a1 == ab1
            g_F = sp(rows, ROT_DIM, f"g_F{it}")
            ops.split_colsum(dF, rows, ROT_DIM, am_dF, g_F, sink.view(fu.b[1]), ab1)
            wgrad(h, g_F, fu.w[1], hid, ROT_DIM, a1)
            dh = torch.empty(rows, hid, dtype=torch.float32, device=dev)
            ops.linear_dgrad_split(g_F, wf1[1], dh, rows, hid, ROT_DIM, relu_mask_sp=h, out_absmax=slot(f"am_dh{it}"))     # (g W) * (h > 0)
            # fuser layer 1: hidden <- the built input
            a0, ab0 = wr.acc(fu.w[0]), wr.acc(fu.b[0])
            assert a0 == ab0
            g_h = sp(rows, hid, f"g_h{it}")
            ops.split_colsum(dh, rows, hid, slot(f"am_dh{it}"), g_h, sink.view(fu.b[0]), ab0)
            wgrad(xf, g_h, fu.w[0], kin, hid, a0)
            dXn = torch.empty(rows, kin, dtype=torch.float32, device=dev)
            ops.linear_dgrad_split(g_h, wf0[1], dXn, rows, kin, hid)
            if not v.share_weights:
                sink.publish(hd.parameters() + fu.parameters())
        dlift = None
        if dXn is not None:
            # iteration 0 read the partner VIEW's lifted feature: sum the directions per source view (and the last image-feature terms)
            dlift = torch.empty(V * B, ROT_DIM, dtype=torch.float32, device=dev)
            ops.fuse_unbuild(None, dXn, rel_fuse, ix["vj"], ix["vi"], dlift, da, da_live, V, V, D, B, cf, NV)
            da_live = True
        return dlift, da_live

    # ---------------------------------------------------------------- backward
    def backward(self, tape: dict, d_lifted: Optional[Tensor], d_feats: Optional[Tensor], d_preds: Optional[Tensor],
                 sink: GradSink, side=None) -> Tensor:
        """Gradients wrt the three outputs (None = zero) -> d(img_feat) [V,B,Cf]; parameter gradients
        go to ``sink`` and are published iteration I-1 ... 0 (shared weights: once, after iteration 0),
        then the lifter.  The kernel family, the weight copies and the shapes are those of tape["call"] - the forward that
        wrote the tape - whatever a later forward (a small validation batch, another compute_dtype) ran on."""
        call: HeadCall = tape["call"]
        V, B, cf, v = call.V, call.B, self.cf, self.v
        if tape.get("wprep_versions") is not None and tape["wprep_versions"] != self._wprep_versions:
            raise RuntimeError("backward of a tape whose sp weight copies were overwritten by a later forward with DIFFERENT "
                               "weights (forward, optimizer step, forward, then backward of the first call): run backward "
                               "before the weights change")
        img_feat = tape["img_feat"]
        dev = img_feat.device
        wr = _Written(sink, side)
        # "a" = what every fuser / head input starts with: image features, or (share_feature) the lifted ones
        da = torch.empty(V, B, ROT_DIM if v.share_feature else cf, dtype=torch.float32, device=dev)
        if call.family is Family.SPLIT:
            dlift, da_live = self._backward_split(tape, d_feats, d_preds, sink, wr, da)
        else:
            dlift, da_live = self._backward_fp32(tape, d_feats, d_preds, sink, wr, da)
        if v.share_weights:
            sink.publish(self.heads[0].parameters() + self.fusers[0].parameters())
        # what every backward ends with: the upstream and (share_feature) the input-side gradients of the lifted features,
        # the lifter's backward into d(img_feat)
        if d_lifted is not None:
            ext = d_lifted.reshape(V * B, ROT_DIM).contiguous()
            if dlift is not None:
                ops.axpby(ext, dlift, 1.0, 1.0)
            else:
                dlift = ext.clone()
        if v.share_feature and da_live:                  # the lifted features ARE the "image features" here
            if dlift is not None:
                ops.axpby(da.view(V * B, ROT_DIM), dlift, 1.0, 1.0)
            else:
                dlift = da.view(V * B, ROT_DIM)
        dimg = da if not v.share_feature else torch.empty(V, B, cf, dtype=torch.float32, device=dev)
        dimg_live = da_live and not v.share_feature
        if dlift is not None:
            self.lifter.backward(call, img_feat.reshape(V * B, cf), tape["hl"], dlift, sink, wr,
                                 dx_addend=dimg.view(V * B, cf) if dimg_live else None, dx_out=dimg.view(V * B, cf))
            dimg_live = True
        else:
            self._zero_grads(self.lifter, sink, wr)
        sink.publish(self.lifter.parameters())
        if not dimg_live:
            dimg.zero_()
        return dimg

    def _backward_fp32(self, tape: dict, d_feats: Optional[Tensor], d_preds: Optional[Tensor], sink: GradSink, wr: _Written,
                       da: Tensor):
        """Backward of _forward_fp32, down to the gradient of the lifted features.  Returns (dlift or None, da_live)."""
        call: HeadCall = tape["call"]
        V, B, D, cf, NV, v = call.V, call.B, call.D, self.cf, NUM_FEAT_VEC, self.v
        rel = tape["rel"]
        dev = rel.device
        ix = self._indices(V, dev)
        da_live = False
        dF_next: Optional[Tensor] = None
        dlift: Optional[Tensor] = None
        rel_fuse = None if (v.ignore_rotmat or v.encode_rotmat) else rel

        def split_input_grad(dX: Tensor, ld: int, rel_b, scales, src_idx, dsrc: Tensor):
            """dX of a fuser / head input -> da (+= over directions) and the gradient of the feature operand."""
            nonlocal da_live
            if v.share_feature:
                da_dir = torch.empty(D * B, ROT_DIM, dtype=torch.float32, device=dev)
                ops.paircat_bwd(dX, rel_b, scales, src_idx, da_dir, dsrc, B, D, NV)
                ops.segment_sum(da_dir, ROT_DIM, ROT_DIM, ix["vi"], da, B, D, V, da_live)
            else:
                ops.segment_sum(dX, ld, cf, ix["vi"], da, B, D, V, da_live)
                if ld == cf + ROT_DIM:
                    ops.rotcat_bwd(dX, rel_b, src_idx, dsrc, B, D, cf, NV)
                else:
                    ops.rotcat_ext_bwd(dX, ld, rel_b, src_idx, dsrc, B, D, cf, NV)
            da_live = True

        for it in range(call.I - 1, -1, -1):
            X, Hf, Xh, Hh, scales = tape["saved"][it]
            dF = dF_next
            if d_feats is not None:
                ext = d_feats[it].reshape(D * B, ROT_DIM).contiguous()
                if dF is None:
                    dF = ext.clone()
                else:
                    ops.axpby(ext, dF, 1.0, 1.0)
            gen_f, gen_h = (X, Xh) if call.fused_in else (None, None)
            if d_preds is not None:
                gp = d_preds[it].reshape(D * B, 2).contiguous()
                dXh = self.heads[it].backward(call, None if gen_h else Xh, Hh, gp, sink, wr, gen=gen_h)
                dFh = torch.empty(D * B, ROT_DIM, dtype=torch.float32, device=dev)
                split_input_grad(dXh, self.hin, None, None, ix["ident"], dFh)
                if dF is None:
                    dF = dFh
                else:
                    ops.axpby(dFh, dF, 1.0, 1.0)
            else:
                self._zero_grads(self.heads[it], sink, wr)
            dF_next = None
            if dF is None:
                self._zero_grads(self.fusers[it], sink, wr)
            else:
                dX = self.fusers[it].backward(call, None if gen_f else X, Hf, dF, sink, wr, gen=gen_f)
                if it > 0:
                    dF_next = torch.empty(D * B, ROT_DIM, dtype=torch.float32, device=dev)
                    split_input_grad(dX, self.kin, rel_fuse, scales, ix["partner"], dF_next)
                else:
                    tmp = torch.empty(D * B, ROT_DIM, dtype=torch.float32, device=dev)
                    split_input_grad(dX, self.kin, rel_fuse, scales, ix["ident"], tmp)
                    dlift = torch.empty(V * B, ROT_DIM, dtype=torch.float32, device=dev)
                    ops.segment_sum(tmp, ROT_DIM, ROT_DIM, ix["vj"], dlift, B, D, V, False)
            if not v.share_weights:
                sink.publish(self.heads[it].parameters() + self.fusers[it].parameters())
        return dlift, da_live

    @staticmethod
    def _zero_grads(m: _Mlp, sink: GradSink, wr: _Written):
        for p in m.parameters():
            if not wr.acc(p):
                sink.view(p).zero_()
