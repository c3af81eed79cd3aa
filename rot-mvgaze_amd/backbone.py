"""ResNet-18/50 backbone over all views at once, forward and backward, on the HIP kernels.

What it replaces: ``self._feat_extractor(img_k)`` for every view k
(/root/reference/models/rot_mv.py:124-128,196-197 -> /root/reference/models/resnet.py:261-275 with
BasicBlock :80-96 / Bottleneck :128-148).  The reference runs one backbone pass per view; here
all V views go through each kernel launch as V *groups* - BatchNorm statistics stay per group and
running statistics are updated once per group in view order, so results equal V separate passes.

Data layout in HBM: activations NHWC ``[V][B][H][W][C]``; per conv+BN unit the tape keeps the raw conv output ``y`` (BN
backward needs x-hat) and the post-activation ``out`` (next conv's input, ReLU mask).

Three kernel families run a unit's conv (``Family``), each with a stem form of its own:
* FP32   the fp32-MFMA kernels: fp32 NHWC activations, the weights are the PyTorch parameters themselves in channels_last
         (= KRSC); the 3-channel stem reads an image padded to 4 channels;
* SPLIT  the split-operand kernels: an fp32 value held as two fp16 pieces ("sp") with a per-tensor 2^-k (``.sinv``), the
         weights as per-step sp copies; the stem in row-window form (``stem_rw``);
* BF16   the bf16 kernels: bf16 activations, per-step bf16 weight copies; the stem on 8-channel taps or in its folded
         row-window form (``stem_rw``).

Where each decision is made:
* ``plan_call`` decides, once per ``forward`` call and on the host alone, what the call runs on - the 2 GiB guard of the
  split kernels, the range guard of inference, the stem's form - and returns the frozen ``Call`` record that every helper
  takes as an argument and that the tape keeps;
* ``unit_family(call, c)`` is the one rule that gives conv ``c`` its family.  Whether a unit's OUTPUT is stored in sp is a
  property of the call (``Call.sp``), not of its conv: the fp32-MFMA stem of a split call writes an sp pooled map;
* every stage - conv launch, statistics partials, weights operand, apply form, stem tail, weight gradient, backward-data,
  the BatchNorm-backward passes, the stem's pool backward - is one ``if family`` chain;
* the backward reads the family from the tape (``_Unit.family`` / ``_Unit.stem_rw``), never from what the Backbone object
  is set to by then; the hand-offs between launches are named tuples (``_Apply``, ``_PendingDy``, ``_FusedSums``, ``_Pool``).
"""
from __future__ import annotations

import enum
import math
import os
from dataclasses import dataclass
from typing import Callable, Dict, List, NamedTuple, Optional

import numpy as np
import torch

from . import ops
from ._lib import ConvDesc
from .arch import RANGE_OVER_BITS, BackboneSpec, ConvSpec, backbone_spec, range_unit_names

Tensor = torch.Tensor
BN_EPS, BN_MOMENTUM = 1e-5, 0.1          # nn.BatchNorm2d defaults (resnet.py:185)
IMAGE_MEAN, IMAGE_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)      # main.py:38-39


BN_APPLY_DGRAD_MAX_COUT = 512      # the merged launch keeps the unit's 5 x cout BatchNorm constants in LDS


def bn_apply_dgrad_eligible(c: ConvSpec, *, split: bool, trained: bool, fused_in: bool, carries_reduce: bool,
                            need_dimg: bool = False) -> bool:
    """Whether unit ``c``'s BatchNorm-backward apply pass is formed inside its own backward-data launch
    (mvg_conv_dgrad_split_bnapply_bnreduce) instead of running as a pass of its own.  All of:
    split path and a training tape (not bf16, not MVG_SPLIT=0, not eval-mode BatchNorm, not a d(img) backward);
    a 1x1 / stride 1 / pad 0 unit whose backward-data GEMM has ONE column tile (cin 64 or 128: every dy element is then
    consumed by exactly one workgroup) and whose constants fit the kernel's table;
    ``fused_in``: its gradient arrived masked, with the fused sums and a ready dy scale (``_Unit.fused_s12``);
    ``carries_reduce``: its backward-data launch carries the fused reduce of the unit below."""
    return bool(split and trained and not need_dimg and fused_in and carries_reduce
                and c.k == 1 and c.stride == 1 and c.pad == 0 and c.cin in (64, 128)
                and c.cout % 32 == 0 and c.cout <= BN_APPLY_DGRAD_MAX_COUT)


def bn_apply_dgrad_units(spec: BackboneSpec, *, split: bool = True, bf16: bool = False, training: bool = True,
                         need_dimg: bool = False, fuse_bn_split: bool = True, enabled: bool = True) -> List[str]:
    """The conv names of ``spec`` that take the merged launch, in backward order: Backbone.backward's decision over the
    architecture plan alone (no GPU).  It is taken for a block's LAST unit: that unit receives a fused gradient from the block
    above (its first conv's backward-data launch, or its downsample branch's) - the network's last block gets its gradient
    from the average pool - and its own launch carries the reduce of the unit below it."""
    on = enabled and split and not bf16 and fuse_bn_split
    nb = len(spec.blocks)
    return [blk.convs[-1].name for bi, blk in reversed(list(enumerate(spec.blocks)))
            if bn_apply_dgrad_eligible(blk.convs[-1], split=on, trained=training, fused_in=bi < nb - 1,
                                       carries_reduce=len(blk.convs) > 1, need_dimg=need_dimg)]


BN_APPLY_FPROP_MAX_CIN = 512       # the merged forward launch keeps the producer's (and the residual's) scale / shift in LDS


def bn_apply_fprop_eligible(producer: ConvSpec, consumer: ConvSpec, *, split: bool, trained: bool, residual: bool = True,
                            relu: bool = True, single_stage: bool = True) -> bool:
    """Whether the BatchNorm apply pass of ``producer`` - a residual block's LAST unit - is formed inside the forward launch of
    ``consumer`` - the NEXT block's first conv (mvg_conv_fprop_split_bnapply) - instead of running as a pass of its own.  All of:
    split path and a training forward on batch statistics (not bf16, not MVG_SPLIT=0, not eval-mode BatchNorm);
    the producer adds a residual and applies the ReLU;
    the consumer is 1x1 / stride 1 / pad 0 with cout 64 or 128: its forward GEMM has ONE column tile, so every element of the
    block output is consumed by exactly one workgroup; cin <= 512: the constants fit the kernel's table;
    ``single_stage``: the launch plan gives the consumer the single-stage K loop (ops.conv_fprop_split_stages: the merged launch
    has no two-stage form)."""
    return bool(split and trained and residual and relu and single_stage
                and consumer.k == 1 and consumer.stride == 1 and consumer.pad == 0 and consumer.cout in (64, 128)
                and consumer.cin == producer.cout and consumer.cin % 32 == 0 and consumer.cin <= BN_APPLY_FPROP_MAX_CIN)


def bn_apply_fprop_pairs(spec: BackboneSpec, *, split: bool = True, bf16: bool = False, training: bool = True, enabled: bool = True,
                         single_stage: Optional[Callable[[ConvSpec], bool]] = None) -> List[tuple]:
    """The (producer, consumer) conv names of ``spec`` that take the merged forward launch, in forward order: Backbone.forward's
    decision over the architecture plan alone (no GPU).  single_stage(consumer) answers the launch-plan condition, which
    depends on the batch and the device (None: met - every such launch of a C3 / C4 step is single-stage)."""
    on = enabled and split and not bf16
    return [(a.convs[-1].name, b.convs[0].name) for a, b in zip(spec.blocks[:-1], spec.blocks[1:])
            if bn_apply_fprop_eligible(a.convs[-1], b.convs[0], split=on, trained=training,
                                       single_stage=True if single_stage is None else single_stage(b.convs[0]))]


class GradSink:
    """Where parameter gradients go.  ``view(p)`` returns the tensor the kernels write into and
    ``accumulate(p)`` says whether they must add to it; ``publish(ps)`` is called once a group of
    parameters has its final gradient (in grad-ready order: DP buckets hang off this).  ``wants(p)`` is False for a
    parameter this backward owes no gradient (``requires_grad = False``): a launch that would write its gradient alone is
    not made, and ``publish`` leaves it out."""

    def view(self, p: torch.nn.Parameter) -> Tensor:
        raise NotImplementedError

    def wants(self, p: torch.nn.Parameter) -> bool:
        return True

    def accumulate(self, p: torch.nn.Parameter) -> bool:
        raise NotImplementedError

    def publish(self, ps: List[torch.nn.Parameter]) -> None:
        raise NotImplementedError


class Family(enum.Enum):
    """The kernel family that runs a unit's conv (see the module docstring)."""
    FP32 = 0      # fp32-MFMA kernels (conv_igemm.hip)
    SPLIT = 1     # split-operand kernels (conv_split.hip): operands (x_in, out, dy, w) in sp
    BF16 = 2      # bf16 kernels (conv_bf16.hip)


class Call(NamedTuple):
    """One Backbone.forward call: what plan_call decided, plus the per-step operands forward() makes (wprep, act_sinv).
    Passed down explicitly and kept on the tape; nothing of it lives on the Backbone object."""
    V: int
    B: int
    H: int
    W: int
    training: bool
    keep_tape: bool
    bf16: bool
    split: bool                 # the split kernels may serve this call (off: MVG_SPLIT=0, the 2 GiB guard, a tripped range guard)
    sp: bool                    # the activations of this call are stored in sp: training steps and folded inference of a split call
    stem_rw: bool               # the stem runs in row-window form (Backbone.stem_rowwindow)
    taped: bool                 # through _forward_taped (training, a tape, unfolded bf16 inference); else the folded _forward_infer
    guard: Optional[str]        # split_eval_guard where it applies (folded fp32 inference), else None
    range_live: bool            # the ranged launches are in use
    need_dimg: bool
    boundary: int               # Backbone._boundary (-1 without a tape)
    wprep: Optional[Dict[str, tuple]] = None        # conv name -> this step's (w, w_t) copies, when ONE launch made them
    act_sinv: Optional[Dict[str, Tensor]] = None    # conv name -> its output's 1-element 2^-k slot (sp training steps)
    train_step: Optional[bool] = None   # a training step (None: = training); differs from ``training`` - BatchNorm on batch
                                        # statistics - for a frozen-BatchNorm step: training False, train_step True


def plan_call(spec: BackboneSpec, *, V: int, B: int, H: int, W: int, training: bool, keep_tape: bool, raw: bool = False,
              augment: bool = False, need_dimg: bool = False, boundary: int = -1, bf16: bool = False, split: bool = True,
              split_eval: bool = True, split_eval_guard: Optional[str] = None, stem_rowwindow: bool = True,
              batch_weight_prep: bool = True, bf16_fold_eval: bool = True, guard_scale: int = 1, tripped: bool = False,
              capturing: bool = False, train_step: Optional[bool] = None, split_frozen: bool = False) -> Call:
    """The size and mode decisions of one forward call, from shapes and flags alone (no tensor, no device).  raw: uint8
    patches; augment: an input augment is set; tripped: an earlier "fallback" call overflowed (Backbone._range_tripped);
    capturing: the stream is being captured; the other flags are the Backbone attributes of the same names.
    training: BatchNorm on batch statistics; train_step (None: = training): the call is a training step - the augment is
    applied and raw patches with one are accepted on the bf16 path.  A frozen-BatchNorm step is training False, train_step
    True: it has no statistics, so no row-window stem and no sp storage, exactly like a taped eval forward - unless
    split_frozen (Backbone.split_frozen) is set: a frozen step of the fp32 model that keeps a tape, wants no d(img) and passes
    the 2 GiB guard then stores its activations in sp (the scales come from the conv launches' statistics partials:
    ops.bn_frozen_finalize) and takes the row-window stem under the conditions a train-mode step does.  Everywhere else -
    eval-mode tapes, need_dimg, the bf16 path, MVG_SPLIT=0, the guard - the flag is inert."""
    step = training if train_step is None else bool(train_step)
    if bf16 and raw and (step or keep_tape) and not (step and augment):
        raise NotImplementedError("raw uint8 input with the bf16 path is served for inference only (model.eval() under "
                                  "torch.no_grad()) and for training steps with model.input_augment (augment.TrainAugment; the "
                                  "identity augment for un-augmented steps): else normalise to fp32 NCHW first")
    # The split kernels address one view of an sp tensor (4 bytes per element) with 32-bit offsets: the largest one
    # (layer1's output: (H/4) x (W/4) x 64 or 256 channels per image) must stay below 2 GiB, or this call runs on the
    # fp32-MFMA kernels (64-bit row offsets there; B <= 668 per view at 224 x 224 with ResNet-50)
    biggest_view_elems = B * ((H + 3) // 4) * ((W + 3) // 4) * spec.blocks[0].convs[-1].cout
    split = split and 4 * biggest_view_elems * guard_scale < 0x7FFFFFF0
    infer = not (training or keep_tape or bf16)         # the folded fp32 inference forward: what split_eval_guard covers
    if split_eval_guard not in (None, "record", "fallback"):
        raise ValueError(f"split_eval_guard must be None, 'record' or 'fallback' (got {split_eval_guard!r})")
    guard = split_eval_guard if infer else None
    if guard == "fallback" and capturing:
        raise RuntimeError("split_eval_guard = 'fallback' reads the range record on the host and cannot run while the stream "
                           "is capturing: capture with 'record' and check overflowed() after the replay")
    if guard == "fallback" and tripped:
        split = False                        # an earlier call overflowed: fp32-MFMA kernels until the weights change
    # the stem's form for this call (see stem_rowwindow)
    frozen = False
    if bf16:        # folded windows: width % 4, whole 64-row partials (n * ho * wo / 2), the stem's weights through the batch
        ho, wo = (H - 1) // 2 + 1, W // 2
        stem_rw = (stem_rowwindow and training and W % 4 == 0 and (B * ho * (wo // 2)) % 64 == 0 and batch_weight_prep
                   and spec.stem.k == 7)
    else:
        # a frozen-BatchNorm step on the split kernels (see frozen_split)
        frozen = bool(split_frozen and split and step and not training and keep_tape and not need_dimg)
        stem_rw = (split and stem_rowwindow and (training or frozen) and not need_dimg and W % 2 == 0
                   and batch_weight_prep and 32 * B * H * (W // 2) * 4 < 0x7FFFFFF0)
    taped = training or keep_tape or (bf16 and not bf16_fold_eval)
    # sp storage: training steps of the fp32 model; folded inference with split_eval (an eval-mode tape: fp32-MFMA kernels)
    sp = split and not bf16 and (training or (infer and split_eval) or frozen)
    return Call(V, B, H, W, training, keep_tape, bf16, split, sp, stem_rw, taped, guard,
                range_live=guard is not None and sp, need_dimg=need_dimg, boundary=boundary, train_step=step)


def frozen_split(call: Call) -> bool:
    """Whether ``call`` is a frozen-BatchNorm training step on the split kernels (plan_call's split_frozen): sp storage on the
    running statistics with a tape - the one sp call that is neither a train-mode step nor folded inference."""
    return bool(call.sp and not call.training and call.keep_tape)


def unit_family(call: Call, c: ConvSpec) -> Family:
    """The family that runs conv ``c`` in ``call``: everything on a bf16 call is bf16; every conv of an sp call is split but
    the 3-channel stem, which is fp32-MFMA (on 4-channel taps) unless the row-window form is on; else fp32-MFMA."""
    if call.bf16:
        return Family.BF16
    if call.sp and (c.cin != 3 or call.stem_rw):
        return Family.SPLIT
    return Family.FP32


class _FrozenScales(dict):
    """Call.act_sinv of a frozen step on the split kernels: conv name -> slot as ever, plus ``state``: conv name -> (the unit's
    4-float bound record, the identity's chained bound or None) - downsample units have a record and no slot."""
    state: Dict[str, tuple]


class _Apply(NamedTuple):
    """A residual unit's forward apply pass, handed to the next block's first conv (bn_apply_fprop_eligible)."""
    y: Tensor
    scale: Tensor
    shift: Tensor
    residual: Optional[Tensor]
    residual_affine: Optional[tuple]
    bits: Optional[Tensor]


class _PendingDy(NamedTuple):
    """What the backward-data launch of a unit needs, besides the unit's own tape record, to form the unit's dy in its loader
    (bn_apply_dgrad_eligible): the masked gradient and its sums.  dy's 2^-k is its .sinv."""
    dz: Tensor
    s1: Tensor
    s2: Tensor


class _FusedSums(NamedTuple):
    """BatchNorm-backward sums delivered by the backward-data launch that produced a unit's (masked) gradient."""
    s1: Tensor
    s2: Tensor
    mx: Optional[Tensor] = None       # split: max |dz| per channel
    sinv: Optional[Tensor] = None     # split: the 2^-k of the dy the unit's apply pass will write


class _Pool(NamedTuple):
    """The stem's fused max pool, for its backward."""
    argmax: Tensor
    scale: Tensor
    shift: Tensor
    ho: int
    wo: int
    hp: int
    wp: int


@dataclass(slots=True)
class _Unit:
    """Saved state of one conv + BN (+ReLU) (+residual) for the backward pass."""
    spec: Optional[ConvSpec] = None
    desc: Optional[ConvDesc] = None
    x_in: Optional[Tensor] = None
    y: Optional[Tensor] = None        # the raw conv output (BatchNorm backward needs x-hat)
    out: Optional[Tensor] = None      # the post-activation map (None: never stored - the stem, a deferred downsample branch)
    mean: Optional[Tensor] = None
    invstd: Optional[Tensor] = None
    relu: bool = False
    rows: int = 0
    w: Optional[Tensor] = None        # the backward-data operand: the transposed copy on the bf16 / split kernels
    trained: bool = True              # normalised with batch statistics (False: eval mode, running statistics)
    pool: Optional[_Pool] = None      # the stem: its fused max pool
    relu_affine: Optional[tuple] = None   # ReLU without residual: (scale, shift) - the backward rebuilds the mask from y
    fused_s12: Optional[_FusedSums] = None    # delivered by the backward-data launch that produced this unit's gradient
    relu_bits: Optional[Tensor] = None    # residual units: the ReLU mask as one byte per 16-byte access (ops.bn_apply_bits)
    family: Family = Family.FP32      # what ran the conv in the forward (unit_family): the backward follows it
    stem_rw: bool = False     # the stem in row-window form: x_in is the window operand (split: dy goes out in sp)


class _Fwd(NamedTuple):
    """What Backbone._unit_fwd returns, whatever its mode (members a mode does not produce are None)."""
    out: Tensor                       # the unit's output; the pooled map (pool); the raw conv output y (defer_apply)
    affine: Optional[tuple] = None    # defer_apply: the (scale, shift) the consumer normalises ``out`` with
    pending: Optional[_Apply] = None  # the apply pass handed to next_conv's forward launch (bn_apply_fprop_eligible)


class Backbone:
    _guard_scale = 1          # tests raise it to exercise the 2 GiB guard of the split path without a 2 GiB tensor
    # tests: a list here makes an inference forward (no tape) append, per unit, (spec name, input, residual, output) - for the
    # stem (spec name, input, raw conv output y, pooled map) - references, no copies
    _debug_units: Optional[list] = None

    def __init__(self, depth: int, params: Dict[str, Tensor], prefix: str = "_feat_extractor.0."):
        self.spec: BackboneSpec = backbone_spec(depth, prefix)
        self.p = params                      # name -> Parameter / buffer (live objects)
        self.fc_dim = self.spec.fc_dim
        # Backward-weight kernels are off the critical path (bn_bwd -> dgrad -> bn_bwd ...): they run on a
        # side stream, where their MFMA work overlaps the HBM-bound BatchNorm-backward passes and the
        # stream-K fix-ups of the main stream.  grad_streams lists every stream that writes gradients
        # besides the caller's (the data-parallel reducer waits on them too).
        self.overlap_wgrad = True
        self.overlap_head = True      # the fusion block's weight gradients too (+1.6 %)
        self.wgrad_low_priority = True      # data-parallel runs use an ordinary stream: gradients must not finish last
        self.grad_streams: List[torch.cuda.Stream] = []
        self._wg_stream: Optional[torch.cuda.Stream] = None
        self._wg_low = True
        # storage type of activations / activation gradients / conv operands: fp32 = the parity path (1e-4 vs
        # the reference); bf16 = BASELINE config C5's "bf16 MFMA path" (fp32 master weights, statistics, gradients)
        self.act_dtype = torch.float32
        # residual units record their ReLU mask as bits in the forward apply pass; the backward reduce pass reads
        # those (1/16 of the activation's bytes) instead of the activation (attribute False: read the activation).
        self.relu_bits = True
        # fp32 training steps on the split-operand kernels (conv_split.hip): every conv but the 3-channel stem reads its
        # operands as two fp16 pieces per fp32 value and runs three fp16 MFMAs per product - fp32-accurate (the 1e-4
        # parity path).  MVG_SPLIT=0: the fp32-MFMA kernels everywhere.
        self.split = os.environ.get("MVG_SPLIT", "1") != "0"
        # split and bf16 paths: the BatchNorm-backward reduce pass of a unit rides on the backward-data launch that
        # produces its output gradient (every unit but the stem and the last one): the staged epilogue already holds 8
        # channels of a row per lane, reads y (and the mask bits) with 16-byte accesses, stores the masked gradient and
        # leaves one partial per row tile; a stride-2 launch's parity classes each bring theirs, the classes a 1x1
        # stride-2 filter never touches as epilogue-only tiles.  (attribute False: separate reduce passes - the tests
        # compare the two.)
        self.fuse_bn_split = True
        # split path, training: a 1x1 stride-1 unit whose backward-data GEMM has one column tile (ResNet-50's layer1 / layer2
        # conv3) forms its dy in that launch's loader (bn_apply_dgrad_eligible; mvg_conv_dgrad_split_bnapply_bnreduce): no
        # apply pass, the sp dy written once for the weight gradient.  (attribute False: the apply pass and the plain launch -
        # the same bits; the tests and the A/B runs compare the two.)
        self.fuse_bn_apply_dgrad = True
        # split path, training: a residual block's output whose first reader is the next block's 1x1 stride-1 conv1 with one column
        # tile (ResNet-50's layer1 / layer2: six block outputs) is formed by that conv's forward loader (bn_apply_fprop_eligible;
        # mvg_conv_fprop_split_bnapply): no apply pass, the sp output written once for its later readers.  (attribute False: the
        # apply pass and the plain launch - the same bits; the tests and the A/B runs compare the two.)
        self.fuse_bn_apply_fprop = True
        # split path, training: the 7x7 stem on the split kernels too, in its "row-window" form (mvg_stem_fprop_split: the
        # image rewritten as [.., W/2, 8 columns x 4 channels] windows, a 7 x 1 filter over 32 channels, K = 224) instead
        # of the fp32-MFMA kernel on 4-channel taps (K = 196 at a fifth of the matrix rate).  Not when the caller wants
        # d(loss)/d(img) (the backward-data launch runs on the fp32 kernel) or the width is odd.
        self.stem_rowwindow = True
        self.split_eval = True      # inference forward on the split kernels too
        # frozen-BatchNorm training steps (training False, train_step True) of the fp32 model on the split kernels as well
        # (plan_call; off: such a step runs on the fp32-MFMA kernels like an eval-mode tape).  Every unit's launch then leaves
        # its statistics partials as in train mode, and ONE launch per unit (ops.bn_frozen_finalize, in place of
        # bn_eval_affine) turns them into the 2^-k of the unit's sp output: running statistics bound nothing, the conv's own
        # batch statistics do.  The backward's reduce forms run on the running (mean, invstd), its apply pass needs no sums.
        self.split_frozen = False
        # Inference on the split kernels stores every activation as two UNSCALED fp16 pieces, and running statistics bound
        # nothing: a checkpoint whose activation reaches 65 520 stores inf, merges to NaN, and a later ReLU can turn that into 0.
        # The guard (folded fp32 inference only; the taped paths and the bf16 path ignore it) makes every sp-producing launch
        # leave max |stored value| - as float bits, an integer atomic max: inf / NaN rank on top - in its word of a record
        # (arch.range_unit_names; same launches, same output bits):
        #   None        today's launches exactly;
        #   "record"    the ranged launches; range_report() / overflowed() read the record (they synchronise, the forward never
        #               does: it can be captured in a graph);
        #   "fallback"  also reads the record after the backbone (one small copy + a synchronisation; not under stream capture) and,
        #               if a tensor overflowed, reruns the call on the fp32-MFMA kernels - the result of split_eval = False, bit
        #               for bit - and stays on them for later inference calls until invalidate_weight_cache() / train().
        self.split_eval_guard: Optional[str] = None
        self._range_record: Optional[Tensor] = None       # int32 [len(range_unit_names)]: a plain attribute, not a buffer
        self._range_slot: Dict[str, int] = {n: i for i, n in enumerate(range_unit_names(depth, prefix))}
        self._range_tripped = False         # "fallback" saw an overflow: inference stays on the fp32-MFMA kernels
        # bf16 path, inference (no tape): BatchNorm on the running statistics, the residual and the ReLU folded into the conv
        # epilogue (mvg_conv_fprop_bf16_affine) - every activation written once and rounded once - the downsample branch
        # stored normalised, and the bf16 weight copies kept between calls.  (attribute False: the training-shaped launches -
        # conv, bn_apply - and a weight cast per call.)
        self.bf16_fold_eval = True
        self._wprep_infer_ok = False          # the persistent bf16 copies hold _wprep_versions and may serve the next inference call
        self._wk_cache: Dict[str, tuple] = {}     # inference: conv name -> (data_ptr, version, sp weights)
        # training: one launch per step makes every conv's bf16 / sp weight copies
        self.batch_weight_prep = True
        self._wprep_state = None
        self._wprep_versions = None
        # split path, training: per-tensor scales of the sp activations (one launch per step: _prepare_act_scales)
        self._ascale_state = None             # (key, device table, records, conv name -> slot, slots)
        self._frozen_plan = None              # frozen steps on the split kernels: [(conv name, identity's conv name or None, has slot)]
        self._wg_defer: Optional[list] = None # backward: (slabs, dw, splits, accumulate) of the split wgrads whose reduce is pending
        self._last_call: Optional[Call] = None    # the record of the last forward call (tests and tools read it through the properties below)
        self._stem_w8 = None

    @property
    def bf16(self) -> bool:
        return self.act_dtype == torch.bfloat16

    @property
    def _split_now(self) -> bool:             # the last call: off when a view's largest sp tensor would exceed 2 GiB
        return self._last_call.split if self._last_call is not None else self.split

    @property
    def _stem_rw(self) -> bool:               # the last call: the stem ran in row-window form
        return self._last_call is not None and self._last_call.stem_rw

    @property
    def _act_sinv(self) -> Optional[Dict[str, Tensor]]:       # the last call: conv name -> its output's 1-element slot
        return self._last_call.act_sinv if self._last_call is not None else None

    # ---------------------------------------------------------------- helpers
    def _prepare_weights(self, dev, family: Family, stem_rw: bool, reuse: bool = False) -> Dict[str, tuple]:
        """The per-step copies of every conv's weights the bf16 / split kernels read (KRSC for fprop, CRSK for
        backward-data), made by ONE launch: destination buffers and the launch's device-resident table of
        (source, destinations, shape) records are built once per parameter placement and reused every step.
        reuse (bf16 inference): no launch when the buffers already hold these parameters - same placement, same version
        counters as _wprep_versions, and nothing invalidated them since (invalidate_weight_cache, train(), any other
        forward).  The buffers then hold exactly what _wprep_versions says, as the tapes that point into them expect."""
        mode = 0 if family is Family.BF16 else 1          # (the launch's own numbering)
        convs = [c for c in self.spec.all_convs() if not (mode == 1 and c.cin == 3 and not stem_rw)]
        key = (mode, stem_rw, str(dev), tuple(self.p[c.name + ".weight"].data_ptr() for c in convs))
        if self._wprep_state is None or self._wprep_state[0] != key:
            out, rows = {}, []
            wstat = torch.zeros(len(convs), 2, dtype=torch.float32, device=dev)      # per conv {max |w| bits, 2^-k} (split path)
            self._stem_w8 = None
            for ci, c in enumerate(convs):
                wsrc = self.p[c.name + ".weight"]
                assert wsrc.is_contiguous(memory_format=torch.channels_last) or (c.k == 1 and wsrc.is_contiguous())
                rs = c.k * c.k
                if mode == 1 and c.cin == 3:
                    # the stem in row-window form: w'[o][r][j][c] = w[o][r][j - 1][c] (j = 0 and c = 3 zero), refreshed from the
                    # parameter below (9408 floats: layout plumbing), then split like a [cout][7][1][32] filter
                    assert c.k == 7
                    self._stem_w8 = torch.zeros(c.cout, 7, 8, 4, dtype=torch.float32, device=dev)
                    wk = ops.sp_empty(c.cout, 7 * 32, device=dev)
                    wk.sinv = wstat[ci, 1:2]
                    out[c.name] = (wk, None)
                    rows.append([self._stem_w8.data_ptr(), wk.data_ptr(), 0, c.cout | (7 << 32), 32 | (32 << 32), wstat[ci].data_ptr()])
                    continue
                if mode == 0 and c.cin == 3 and stem_rw:
                    # bf16 path, folded windows (16 columns x 4 channels serve two output columns): two copies of the filter,
                    # w'[par * cout + o][r][j][c] = w[o][r][j - 1 - 2 par][c], cast like a [2 cout][7][1][64] filter
                    assert c.k == 7
                    self._stem_w8 = torch.zeros(2 * c.cout, 7, 16, 4, dtype=torch.float32, device=dev)
                    wk = torch.empty(2 * c.cout, 7, 1, 64, dtype=torch.bfloat16, device=dev)
                    out[c.name] = (wk, None)
                    rows.append([self._stem_w8.data_ptr(), wk.data_ptr(), 0, (2 * c.cout) | (7 << 32), 64 | (64 << 32), wstat[ci].data_ptr()])
                    continue
                if mode == 1:
                    wk = ops.sp_empty(c.cout, rs * c.cin, device=dev)
                    wt = ops.sp_empty(c.cin, rs * c.cout, device=dev)
                    wk.sinv = wt.sinv = wstat[ci, 1:2]
                    cin_pad = c.cin
                else:
                    cin_pad = 8 if c.cin == 3 else c.cin
                    wk = torch.empty(c.cout, c.k, c.k, cin_pad, dtype=torch.bfloat16, device=dev)
                    wt = None if c.cin == 3 else torch.empty(cin_pad, c.k, c.k, c.cout, dtype=torch.bfloat16, device=dev)
                out[c.name] = (wk, wt)
                rows.append([wsrc.data_ptr(), wk.data_ptr(), wt.data_ptr() if wt is not None else 0, c.cout | (rs << 32),
                             c.cin | (cin_pad << 32), wstat[ci].data_ptr()])
            table = torch.tensor(rows, dtype=torch.int64).to(dev)            # once per placement (a host-to-device copy)
            self._wprep_state = (key, out, table, len(rows), mode, wstat)
        elif (reuse and self._wprep_infer_ok and
              self._wprep_versions == tuple(self.p[c.name + ".weight"]._version for c in self.spec.all_convs())):
            return self._wprep_state[1]
        _, out, table, n, mode, wstat = self._wprep_state
        self._wprep_infer_ok = reuse
        if mode == 1:
            wstat.zero_()                                  # the max |w| slots are atomicMax targets
            if self._stem_w8 is not None:
                self._stem_w8[:, :, 1:, :3].copy_(self.p[self.spec.stem.name + ".weight"].detach().permute(0, 2, 3, 1))
        elif self._stem_w8 is not None:
            wsrc, co = self.p[self.spec.stem.name + ".weight"].detach().permute(0, 2, 3, 1), self.spec.stem.cout
            self._stem_w8[:co, :, 1:8, :3].copy_(wsrc)
            self._stem_w8[co:, :, 3:10, :3].copy_(wsrc)
        ops.weights_prep_batch(table, n, mode)
        # the copies live in persistent buffers that the next forward overwrites: remember which parameter versions
        # they hold, so that the backward of an OLDER tape can tell (tapes keep pointers into these buffers)
        self._wprep_versions = tuple(self.p[c.name + ".weight"]._version for c in self.spec.all_convs())
        return out

    def _prepare_act_scales(self, dev, B: int, H: int, W: int) -> Dict[str, Tensor]:
        """The 2^-k of every sp activation this training step stores (each unit's output, the stem's pooled map), by ONE
        single-workgroup launch (ops.act_scales) from a bound that depends on parameters and shapes only:
            bound(unit) = max_c(|gamma_c| sqrt(n - 1) + |beta_c|),   n = B Ho Wo  (a z-score of n samples is <= sqrt(n - 1)),
            bound(block output) = bound(last unit) + bound(identity: previous block's output, or the downsample BatchNorm).
        The device table of (gamma, beta, channels, sqrt(n - 1), identity record, slot) records is built once per
        (placement, B, H, W); the slots are a fresh tensor per step, kept alive by the sp tensors that carry its 1-element
        views as ``.sinv``.  Returns conv name -> slot view.  No pass over an activation, no atomics, no host synchronisation."""
        s = self.spec
        convs = s.all_convs()
        key = (str(dev), B, H, W, tuple((self.p[c.bn + ".weight"].data_ptr(), self.p[c.bn + ".bias"].data_ptr()) for c in convs))
        if self._ascale_state is None or self._ascale_state[0] != key:
            rec, slot_of = [], {}

            def size(h, c):
                return (h + 2 * c.pad - c.k) // c.stride + 1

            def add(c, n, ident, has_slot):
                slot = -1
                if has_slot:
                    slot = slot_of[c.name] = len(slot_of)
                rec.append((self.p[c.bn + ".weight"].data_ptr(), self.p[c.bn + ".bias"].data_ptr(), c.cout,
                            math.sqrt(max(n - 1, 0)), ident, slot))
                return len(rec) - 1
            h, w = size(H, s.stem), size(W, s.stem)
            prev = add(s.stem, B * h * w, -1, True)          # the pooled map: max pool and ReLU do not raise the unit's bound
            h, w = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
            for blk in s.blocks:
                hb, wb = h, w
                for c in blk.convs[:-1]:
                    hb, wb = size(hb, c), size(wb, c)
                    add(c, B * hb * wb, -1, True)
                ident = prev
                if blk.downsample is not None:           # its normalised map is never stored: a bound, no slot
                    ident = add(blk.downsample, B * size(h, blk.downsample) * size(w, blk.downsample), -1, False)
                c = blk.convs[-1]
                hb, wb = size(hb, c), size(wb, c)
                prev = add(c, B * hb * wb, ident, True)
                h, w = hb, wb
            items = np.array(rec, dtype=np.dtype([("gamma", "<i8"), ("beta", "<i8"), ("c", "<i4"), ("sqrt_n1", "<f4"),
                                                  ("ident", "<i4"), ("slot", "<i4")]))
            table = torch.from_numpy(items.view("<i8").reshape(len(rec), 4).copy()).to(dev)   # once per placement and shape
            self._ascale_state = (key, table, len(rec), slot_of, len(slot_of))
        _, table, n, slot_of, n_slots = self._ascale_state
        slots = torch.empty(n_slots, dtype=torch.float32, device=dev)
        ops.act_scales(table, n, slots)
        views = slots.split(1)
        return {name: views[i] for name, i in slot_of.items()}

    def _prepare_frozen_scales(self, dev):
        """The slots and bound records of a frozen-BatchNorm step on the split kernels.  Nothing is computed here: every unit's
        ops.bn_frozen_finalize launch fills its own slot from its conv's statistics partials and chains its bound to its
        identity's - the previous block's last unit (first block: the stem), or the block's downsample unit, which has a bound
        and no slot.  Both tensors are fresh per step (the records arrive zeroed: one fill), the slots kept alive by the sp
        tensors that carry their 1-element views as ``.sinv``.  Returns a _FrozenScales."""
        s = self.spec
        if self._frozen_plan is None:
            plan = [(s.stem.name, None, True)]
            prev = s.stem.name
            for blk in s.blocks:
                plan += [(c.name, None, True) for c in blk.convs[:-1]]
                ident = prev
                if blk.downsample is not None:
                    plan.append((blk.downsample.name, None, False))
                    ident = blk.downsample.name
                plan.append((blk.convs[-1].name, ident, True))
                prev = blk.convs[-1].name
            self._frozen_plan = plan
        plan = self._frozen_plan
        records = torch.zeros(len(plan), 4, dtype=torch.float32, device=dev)
        slots = torch.empty(sum(1 for _, _, has in plan if has), dtype=torch.float32, device=dev).split(1)
        row = {name: i for i, (name, _, _) in enumerate(plan)}
        sinv, state, k = _FrozenScales(), {}, 0
        for name, ident, has in plan:
            if has:
                sinv[name] = slots[k]
                k += 1
            state[name] = (records[row[name]], records[row[ident]][2:3] if ident is not None else None)
        sinv.state = state
        return sinv

    def invalidate_weight_cache(self):
        """Forget the inference path's cached sp (bf16 path: bf16) copies of the conv weights.  The cache is keyed on each parameter's
        (data_ptr, version counter); writes that bypass the counter - ``p.data.copy_()`` / ``p.data.mul_()`` (EMA,
        clipping) or writes to ``model.param_arena()`` - must be followed by this call (or by
        ``torch.autograd.graph.increment_version(p)``), otherwise ``torch.no_grad()`` inference keeps using the old
        weights.  ``model.train()`` and every training forward clear it too."""
        self._wk_cache.clear()
        self._wprep_infer_ok = False          # bf16 path: the next inference call casts the weights again
        self._range_tripped = False           # new weights: the guarded forward tries the split kernels again

    def _range_words(self) -> Tensor:
        if self.split_eval_guard is None or self._range_record is None:
            raise RuntimeError("no activation range record: set split_eval_guard to 'record' or 'fallback' and run an inference forward")
        return self._range_record.cpu()        # (synchronises)

    def range_report(self) -> Dict[str, float]:
        """{conv name: max |activation| of the sp tensor its unit stored} of the last guarded inference forward, in forward
        order (inf / nan when the fp32 value was); all zeros when that call did not run on the split kernels.  Synchronises."""
        vals = self._range_words().view(torch.float32).tolist()
        return {n: vals[i] for n, i in self._range_slot.items()}

    def overflowed(self) -> List[str]:
        """The units of range_report() whose tensor reached 65 520 (an fp16 piece became inf), in forward order.  Synchronises."""
        words = self._range_words().tolist()
        return [n for n, i in self._range_slot.items() if words[i] >= RANGE_OVER_BITS]

    def bn_count_buffers(self) -> List[Tensor]:
        return [self.p[c.bn + ".num_batches_tracked"] for c in self.spec.all_convs()]

    # ---------------------------------------------------------------- forward
    def _conv_weights(self, call: Call, c: ConvSpec, d: ConvDesc, family: Family, need_transposed: bool):
        """(w, w_t): the KRSC weight operand of conv ``c`` and its transposed copy for backward-data (or None).  SPLIT / BF16:
        this step's copies when ONE launch at the start of forward() made them (call.wprep), else a split / cast per call;
        FP32: the fp32 parameter itself."""
        if family is not Family.FP32 and call.wprep is not None:
            return call.wprep[c.name]
        wsrc = self.p[c.name + ".weight"].detach()
        if family is Family.FP32 and c.cin == 3:                          # the 3-channel stem padded to 4 channels
            w4 = torch.zeros(c.cout, c.k, c.k, 4, dtype=torch.float32, device=wsrc.device)
            w4[..., :3].copy_(wsrc.permute(0, 2, 3, 1))                   # 9408 floats: layout plumbing
            return w4, None
        assert wsrc.is_contiguous(memory_format=torch.channels_last) or (c.k == 1 and wsrc.is_contiguous()), \
            f"{c.name}.weight must be channels_last (KRSC)"
        if family is Family.FP32:
            return wsrc, None
        if family is Family.SPLIT:
            return ops.split_weights(d, wsrc, need_transposed=need_transposed)
        # one cast of the fp32 master weights per step: KRSC for fprop, CRSK (transposed) for backward-data
        return ops.cast_weights_bf16(d, wsrc, c.cin, need_transposed=need_transposed and c.cin != 3)

    def _unit_infer(self, call: Call, c: ConvSpec, x: Tensor, H: int, W: int, relu: bool, residual: Optional[Tensor],
                    pool: bool = False) -> Tensor:
        """Folded inference unit (no tape, not training, not the unfolded bf16 form): conv with BatchNorm on the running
        statistics (+ residual) (+ ReLU) in its epilogue - ONE launch, the output written once.  Returns the unit's output;
        pool (the fp32 stem): the max-pooled map, in sp when the split kernels serve the call.
        csrc/session_plan.cpp restates this method (its unit()) and _forward_infer (its block loop) as data, for the fp32
        model (build) and for the bf16 branch (build_bf16): a change to the launches here must be made there too."""
        family, G, N = unit_family(call, c), call.V, call.B
        assert not (family is Family.BF16 and pool)      # the bf16 stem goes through _unit_fwd
        d = ConvDesc.make(G, N, H, W, 4 if c.cin == 3 else c.cin, c.cout, c.k, c.stride, c.pad)
        dev = x.device
        if family is not Family.SPLIT:           # (SPLIT: the cached sp copy below)
            w, _ = self._conv_weights(call, c, d, family, False)
        aff = torch.empty(2, 1, c.cout, dtype=torch.float32, device=dev)
        ops.bn_eval_affine(1, c.cout, self.p[c.bn + ".weight"].detach(), self.p[c.bn + ".bias"].detach(),
                           self.p[c.bn + ".running_mean"], self.p[c.bn + ".running_var"], BN_EPS, aff[0], aff[1])
        scale, shift = aff[0, 0], aff[1, 0]
        if family is Family.SPLIT:
            # the epilogue writes the next conv's sp operand directly (the downsample branch, read only as a residual, stays
            # fp32).  The sp copy of the weights is kept between calls while the parameter is unchanged (its version counter:
            # load_state_dict, optimizer steps - the fused Adam bumps it explicitly - and broadcasts all move it)
            wsrc = self.p[c.name + ".weight"]
            hit = self._wk_cache.get(c.name)
            if hit is not None and hit[0] == wsrc.data_ptr() and hit[1] == wsrc._version:
                wk = hit[2]
            else:
                wk, _ = self._conv_weights(call, c, d, family, False)
                self._wk_cache[c.name] = (wsrc.data_ptr(), wsrc._version, wk)
            out = (ops.sp_empty(G, N, d.ho, d.wo, c.cout, device=dev) if relu
                   else torch.empty(G, N, d.ho, d.wo, c.cout, dtype=torch.float32, device=dev))
            if call.range_live and relu:         # (an sp output: every unit but the downsample branches)
                ops.conv_fprop_split_affine_ranged(d, x, wk, out, scale, shift, residual, relu, self._range_word(c))
            else:
                ops.conv_fprop_split_affine(d, x, wk, out, scale, shift, residual, relu)
            return out
        y = torch.empty(G, N, d.ho, d.wo, c.cout, dtype=self.act_dtype, device=dev)
        if family is Family.BF16:                # y is the unit's output, written once, rounded once
            ops.conv_fprop_bf16_affine(d, x, w, y, scale, shift, residual, relu)
            if self._debug_units is not None:
                self._debug_units.append((c.name, x, residual, y))
            return y
        ops.conv_fprop_affine(d, x, w, y, scale, shift, residual, relu)
        if not pool:
            return y
        pooled = self._pool_plain(y, G, N, d.ho, d.wo, c.cout)
        if call.range_live:                      # (the pooled map of an sp call)
            return ops.split_f32_ranged(pooled, self._range_word(c))
        return ops.split_f32(pooled) if call.sp else pooled

    def _range_word(self, c: ConvSpec) -> Tensor:
        i = self._range_slot[c.name]
        return self._range_record[i:i + 1]

    @staticmethod
    def _pool_plain(a0: Tensor, G: int, N: int, h: int, w: int, c: int) -> Tensor:
        hp, wp_ = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
        x = torch.empty(G, N, hp, wp_, c, dtype=torch.float32, device=a0.device)
        argmax = torch.empty(G, N, hp, wp_, c, dtype=torch.uint8, device=a0.device)       # (written, never read: no backward)
        ops.maxpool_fwd(a0, x, argmax, G * N, h, w, c, hp, wp_)
        return x

    @staticmethod
    def _stats_partials(c: ConvSpec, d: ConvDesc, family: Family, stem_rw: bool):
        """(partials per group, rows per partial) of the batch statistics that the unit's forward launch leaves."""
        if family is Family.BF16:
            if stem_rw:             # two output columns per GEMM row: twice the partials of a forward over n x ho x wo/2 rows
                P, rpp = ops.conv_stats_partials(ConvDesc.make(d.groups, d.n, d.ho, d.wo // 2, 64, 2 * c.cout, 1, 1, 0), True)
                return 2 * P, rpp
            return ops.conv_stats_partials(d, True)
        if family is Family.SPLIT:
            if stem_rw:             # the same row tiles as any split forward with these n, ho, wo
                return ops.conv_stats_partials_split(ConvDesc.make(d.groups, d.n, d.ho, d.wo, 32, c.cout, 1, 1, 0))
            return ops.conv_stats_partials_split(d)
        return ops.conv_stats_partials(d, False)

    def _unit_fwd(self, call: Call, c: ConvSpec, x: Tensor, H: int, W: int, *, relu: bool, residual: Optional[Tensor] = None,
                  tape: Optional[list] = None, pool: bool = False, residual_affine=None, defer_apply: bool = False,
                  next_conv: Optional[ConvSpec] = None, pending_apply: Optional[_Apply] = None) -> _Fwd:
        """conv -> BatchNorm (-> + residual) (-> ReLU), the BatchNorm as passes of its own: batch statistics (training) or
        the running ones (eval mode with a tape; bf16 inference that is not folded; the bf16 inference stem).  Returns _Fwd.
        pool=True (the stem): the 3x3/2 max pool is fused behind the ReLU - out is the pooled map; the normalised map is not stored.
        The non-training pool=True branch on the bf16 path - conv_fprop without statistics, bn_eval_affine over G rows,
        _stem_tail - is restated as the stem of csrc/session_plan.cpp's build_bf16: a change here is made there too.
        defer_apply (the downsample branch): stop after the statistics - out is the raw conv output y and affine its
        (scale, shift): the normalisation is applied by the consumer, the block's last unit, which takes them as
        residual / residual_affine; the normalised downsample map is never written.
        next_conv (a block's last unit: the next block's first conv): when bn_apply_fprop_eligible accepts the pair, this unit's
        apply pass is NOT launched - out is allocated and recorded on the tape as usual, and the next block's first unit
        takes ``pending`` as pending_apply: its forward launch forms, uses and writes ``x`` (= that out)."""
        family = unit_family(call, c)
        stem_rw = c.cin == 3 and call.stem_rw     # x is then the row-window operand (ops.stem_rowwindow_split / _bf16)
        G, N, training, keep = call.V, call.B, call.training, tape is not None
        d = ConvDesc.make(G, N, H, W, (8 if family is Family.BF16 else 4) if c.cin == 3 else c.cin, c.cout, c.k, c.stride, c.pad)
        assert pending_apply is None or (family is Family.SPLIT and not stem_rw)
        assert not stem_rw or call.wprep is not None                # the row-window filter comes from the batched weight prep only
        w, w_t = self._conv_weights(call, c, d, family, keep)
        rows = N * d.ho * d.wo
        # training: (partials per group, rows per partial) of the batch statistics that the conv launch leaves
        # (a frozen step on the split kernels asks for them too: its activation scales come from them)
        partials = self._stats_partials(c, d, family, stem_rw) if (training or frozen_split(call)) else None
        y, stats = self._conv_fwd(c, d, family, stem_rw, x, w, pending_apply, partials)
        mean, invstd, scale, shift = self._bn_fwd_stats(call, c, G, rows, stats, partials)
        out = bits = pool_rec = handed = None
        if defer_apply:
            assert not relu and residual is None and not pool
        elif pool:
            assert relu and residual is None
            out, pool_rec = self._stem_tail(call, c, d, y, scale, shift)
            if self._debug_units is not None and not keep and not training:
                self._debug_units.append((c.name, x, y, out))
        else:
            out, bits, handed = self._apply_fwd(call, c, d, family, y, scale, shift, relu, residual, residual_affine, keep, next_conv)
        if keep:
            # (ReLU without residual: the backward rebuilds the mask from y - saves reading `out` twice)
            tape.append(_Unit(spec=c, desc=d, x_in=x, y=y, out=None if pool else out, mean=mean, invstd=invstd, relu=relu,
                              rows=rows, w=w if family is Family.FP32 else w_t, trained=training, family=family, stem_rw=stem_rw,
                              relu_affine=(scale, shift) if (relu and residual is None and not pool) else None,
                              pool=pool_rec, relu_bits=bits))
        return _Fwd(y, affine=(scale, shift)) if defer_apply else _Fwd(out, pending=handed)

    def _conv_fwd(self, c: ConvSpec, d: ConvDesc, family: Family, stem_rw: bool, x: Tensor, w: Tensor,
                  pending_apply: Optional[_Apply], partials: Optional[tuple]):
        """Stage 1 of _unit_fwd, the conv launch.  Returns (y, stats): the raw conv output and, in training, the partial batch
        statistics per row tile that the launch leaves (else None)."""
        dev = x.device
        y = torch.empty(d.groups, d.n, d.ho, d.wo, c.cout, dtype=self.act_dtype, device=dev)
        stats = None
        if partials is not None:
            stats = torch.empty(d.groups, partials[0], 2, c.cout, dtype=torch.float32, device=dev)
        if family is Family.BF16:
            if stem_rw:
                ops.stem_fprop_bf16(d, x, w, y, stats)
            else:
                ops.conv_fprop(d, x, w, y, None, False, stats)
        elif family is Family.SPLIT:
            if stem_rw:
                ops.stem_fprop_split(d, x, w, y, stats)
            elif pending_apply is not None:
                # x does not exist yet: this launch forms it from the previous block's last unit, then every later reader finds it
                p = pending_apply
                ops.conv_fprop_split_bnapply(d, x, p.y, p.scale, p.shift, p.residual, w, y, stats, p.residual_affine, p.bits)
            else:
                ops.conv_fprop_split(d, x, w, y, stats)
        else:
            ops.conv_fprop(d, x, w, y, None, False, stats)
        return y, stats

    def _bn_fwd_stats(self, call: Call, c: ConvSpec, G: int, rows: int, stats: Optional[Tensor], partials: Optional[tuple]):
        """Stage 2 of _unit_fwd: (mean, invstd, scale, shift) from the launch's partials (training: batch statistics, and the
        running ones updated), else from the running statistics (mean / invstd are then left unfilled) - but for a frozen step
        on the split kernels: one launch writes the eval-mode (scale, shift), mean / invstd := the running values for the
        backward's reduce forms, and from the partials the unit's bound and the 2^-k of its sp output."""
        gamma, beta = self.p[c.bn + ".weight"].detach(), self.p[c.bn + ".bias"].detach()
        rm, rv = self.p[c.bn + ".running_mean"], self.p[c.bn + ".running_var"]
        mean, invstd, scale, shift = torch.empty(4, G, c.cout, dtype=torch.float32, device=gamma.device)
        if frozen_split(call):
            P, rpp = partials
            state, ident = call.act_sinv.state[c.name]
            ops.bn_frozen_finalize(stats, G, P, rpp, rows, c.cout, gamma, beta, rm, rv, BN_EPS, mean, invstd, scale, shift, state,
                                   call.act_sinv.get(c.name), ident)
        elif partials is not None:
            P, rpp = partials
            ops.bn_finalize(stats, G, P, rpp, rows, c.cout, gamma, beta, rm, rv, BN_MOMENTUM, BN_EPS, mean, invstd,
                            scale, shift)
        else:
            ops.bn_eval_affine(G, c.cout, gamma, beta, rm, rv, BN_EPS, scale, shift)
        return mean, invstd, scale, shift

    def _apply_fwd(self, call: Call, c: ConvSpec, d: ConvDesc, family: Family, y: Tensor, scale: Tensor, shift: Tensor, relu: bool,
                   residual: Optional[Tensor], residual_affine, keep: bool, next_conv: Optional[ConvSpec]):
        """Stage 3 of _unit_fwd: the apply pass (+ residual) (+ ReLU), or its hand-off to next_conv's launch.  The output's
        storage follows the call (sp or the activation type).  Returns (out, the ReLU mask bits or None, the _Apply handed on
        or None)."""
        G, rows = d.groups, d.n * d.ho * d.wo
        if call.sp:
            out = ops.sp_empty(G, d.n, d.ho, d.wo, c.cout, device=y.device)
            out.sinv = call.act_sinv[c.name]        # this step's 2^-k of the unit's output (an sp identity brings its own)
            want_bits = keep and relu and residual is not None
            if (next_conv is not None and self.fuse_bn_apply_fprop
                    and bn_apply_fprop_eligible(c, next_conv, split=family is Family.SPLIT, trained=call.training,
                                                residual=residual is not None, relu=relu)
                    and ops.conv_fprop_split_stages(ConvDesc.make(G, d.n, d.ho, d.wo, next_conv.cin, next_conv.cout, 1, 1, 0)) == 1):
                bits = torch.empty(G * rows * c.cout // 4, dtype=torch.uint8, device=y.device) if want_bits else None
                return out, bits, _Apply(y, scale, shift, residual, residual_affine, bits)
            bits = ops.bn_apply_split(y, scale, shift, residual, relu, out, G, rows, c.cout, residual_affine, want_bits=want_bits)
            return out, bits, None
        out = torch.empty_like(y) if keep else y            # inference: normalise in place
        if keep and relu and residual is not None and self.relu_bits:
            return out, ops.bn_apply_bits(y, scale, shift, residual, out, G, rows, c.cout, residual_affine), None
        ops.bn_apply(y, scale, shift, residual, relu, out, G, rows, c.cout, residual_affine)
        return out, None, None

    def _stem_tail(self, call: Call, c: ConvSpec, d: ConvDesc, y: Tensor, scale: Tensor, shift: Tensor):
        """BatchNorm apply + ReLU + 3x3/2 max pool of the stem in one pass, the pooled map stored as the call stores its
        activations.  Returns (pooled map, the _Unit.pool record)."""
        G, N = y.shape[0], y.shape[1]
        hp, wp_ = (d.ho + 2 - 3) // 2 + 1, (d.wo + 2 - 3) // 2 + 1
        argmax = torch.empty(G, N, hp, wp_, c.cout, dtype=torch.uint8, device=y.device)
        if call.sp:
            out = ops.sp_empty(G, N, hp, wp_, c.cout, device=y.device)
            out.sinv = call.act_sinv[c.name]
            ops.bn_relu_maxpool_fwd_split(y, scale, shift, out, argmax, G, N, d.ho, d.wo, c.cout, hp, wp_)
        else:
            out = torch.empty(G, N, hp, wp_, c.cout, dtype=self.act_dtype, device=y.device)
            ops.bn_relu_maxpool_fwd(y, scale, shift, out, argmax, G, N, d.ho, d.wo, c.cout, hp, wp_)
        return out, _Pool(argmax, scale, shift, d.ho, d.wo, hp, wp_)

    def _input_layout(self, call: Call, imgs: List[Tensor], input_bgr: bool, augment=None) -> Tensor:
        """x0, the stem's input operand, one launch per view: row windows straight from the NCHW input when the stem runs in
        row-window form (no NHWC image is built); else the NHWC image padded to 4 (bf16: 8) channels, from raw uint8 patches
        or NCHW fp32 - and the windows from that image for raw input with a row-window stem.  augment (training steps on raw
        patches: an augment.TrainAugment): its launch - ColorJitter, RandomAffine, ToTensor, Normalize, erase - takes the
        place of the preprocess launch; the draws are host work, taken in view order, then image order - or, with a capturable
        augment (draws="device"), one more launch per view (mvg_augment_draw) and no host work at all.  On the bf16 path
        that launch stores the stem's operand itself - the row windows when the stem runs in row-window form, else the NHWC8
        image - rounded once from the fp32 value: one launch per view, no fp32 image in between.
        (The bf16 branch without a row-window stem is restated by csrc/session_plan.cpp's build_bf16.)"""
        V, B, H, W, dev, bf = call.V, call.B, call.H, call.W, imgs[0].device, call.bf16
        raw = imgs[0].dtype == torch.uint8
        direct = call.stem_rw and (not raw or (bf and augment is not None))     # each view's launch writes the windows itself
        if direct and bf:
            x0 = torch.empty(V, B, H, W // 4, 64, dtype=self.act_dtype, device=dev)
        elif direct:
            x0 = ops.sp_empty(V, B, H, W // 2, 32, device=dev)
            x0.sinv = None
        else:
            x0 = torch.empty(V, B, H, W, 8 if bf else 4, dtype=self.act_dtype, device=dev)
        for v, im in enumerate(imgs):
            assert im.shape == imgs[0].shape and im.is_cuda and im.dtype == imgs[0].dtype
            if raw and augment is not None:
                if tuple(im.shape[1:3]) != (H, W):
                    raise ValueError(f"input_augment: {im.shape[1]} x {im.shape[2]} patches with input_size {H} x {W}: a resize "
                                     "after the augmentation is not served (set model.input_size = None, or feed patches of that size)")
                if getattr(augment, "capturable", False):       # draws="device": one more launch, nothing on the host
                    draws = augment.draw_device(B, H, W, dev)
                elif torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("input_augment draws on the host for every step and cannot be captured (graph.GraphedStep): "
                                       "augment outside the captured step (TrainAugment.apply) and feed the result")
                else:
                    draws = augment.draw(B, H, W)
                if bf and direct:
                    augment.launch(im, draws, None, None, input_bgr, dst_rw=x0[v])
                elif bf:
                    augment.launch(im, draws, None, None, input_bgr, dst_nhwc8=x0[v])
                else:
                    augment.launch(im, draws, None, x0[v], input_bgr)
                continue
            if raw:                             # (bf16: no fp32 image in between)
                prep = ops.preprocess_u8hwc_resize_bf16 if bf else ops.preprocess_u8hwc_resize
                prep(im.contiguous(), x0[v], B, im.shape[1], im.shape[2], H, W, IMAGE_MEAN, IMAGE_STD, input_bgr)
                continue
            assert im.dtype == torch.float32
            if direct:
                (ops.stem_rowwindow_bf16 if bf else ops.stem_rowwindow_split_nchw)(im.detach().contiguous(), x0[v])
            else:
                (ops.nchw_to_nhwc8_bf16 if bf else ops.nchw_to_nhwc4)(im.detach().contiguous(), x0[v], B, 3, H, W)
        if call.stem_rw and not direct:                 # raw uint8 input: windows from the normalised NHWC4 image
            x0 = ops.stem_rowwindow_split(x0)
        return x0

    def forward(self, imgs: List[Tensor], training: bool, keep_tape: bool, input_bgr: bool = False,
                input_size: Optional[int] = None, need_dimg: bool = False, input_augment=None,
                train_step: Optional[bool] = None):
        """imgs: V tensors [B,3,H,W] fp32 NCHW (the reference's input format, rot_mv.py:188-189), or
        V raw uint8 [B,H,W,3] face patches, put through test_transform of main.py:50-55 on the GPU
        (ToTensor, Resize((input_size, input_size), antialias=True) when the patch has another size,
        Normalize) - in a training step with input_augment (augment.TrainAugment) through the random
        part of train_transform (main.py:41-49) as well.  The bf16 path takes raw patches for inference and, with
        input_augment, for training steps (the augment launch stores the bf16 stem operand); a training step or a taped
        forward on raw patches without it raises NotImplementedError.  training: BatchNorm on batch statistics; train_step
        (None: = training): this is a training step - the augment is applied and the inference weight copies are dropped.
        A frozen-BatchNorm step (MultiViewGaze.freeze_batchnorm) is training False, train_step True.
        Returns (img_feat [V,B,fc_dim], tape or None)."""
        step = training if train_step is None else bool(train_step)
        V = len(imgs)
        raw = imgs[0].dtype == torch.uint8
        if raw:
            B, Hin, Win, C = imgs[0].shape
            H, W = (input_size, input_size) if input_size else (Hin, Win)
        else:
            B, C, H, W = imgs[0].shape
        assert C == 3
        dev = imgs[0].device
        call = plan_call(self.spec, V=V, B=B, H=H, W=W, training=training, keep_tape=keep_tape, raw=raw,
                         augment=input_augment is not None, need_dimg=need_dimg, boundary=self._boundary(need_dimg) if keep_tape else -1,
                         bf16=self.bf16, split=self.split, split_eval=self.split_eval, split_eval_guard=self.split_eval_guard,
                         stem_rowwindow=self.stem_rowwindow, batch_weight_prep=self.batch_weight_prep,
                         bf16_fold_eval=self.bf16_fold_eval, guard_scale=self._guard_scale, tripped=self._range_tripped,
                         capturing=self.split_eval_guard == "fallback" and torch.cuda.is_current_stream_capturing(),
                         train_step=step, split_frozen=self.split_frozen)
        x0 = self._input_layout(call, imgs, input_bgr, input_augment if (raw and step) else None)
        if step:
            self.invalidate_weight_cache()       # the weights are about to change: drop the inference copies
        wprep = None
        frozen = frozen_split(call)
        if self.batch_weight_prep and (call.bf16 or (call.sp and (training or frozen))):
            wprep = self._prepare_weights(dev, Family.BF16 if call.bf16 else Family.SPLIT, call.stem_rw,
                                          reuse=call.bf16 and self.bf16_fold_eval and not training and not keep_tape)
        # ... and one launch gives every sp activation of the step its scale (x, out and identity carry it as .sinv; the
        # tape's x_in / out keep it for the backward's weight gradients)
        if frozen:        # ... or, on the running statistics, every unit's own finalize launch does (the slots arrive unfilled)
            call = call._replace(wprep=wprep, act_sinv=self._prepare_frozen_scales(dev))
        else:
            call = call._replace(wprep=wprep, act_sinv=self._prepare_act_scales(dev, B, H, W) if (call.sp and training) else None)
        # (V, B and boundary stay as keys of their own: tests and tools read them)
        tape: Optional[dict] = {"units": [], "blocks": [], "call": call, "V": V, "B": B, "boundary": call.boundary} if keep_tape else None
        if keep_tape and wprep is not None:
            tape["wprep_versions"] = self._wprep_versions
        if training:
            torch._foreach_add_(self.bn_count_buffers(), V)       # num_batches_tracked += 1 per view call
        if call.taped:
            x = self._forward_taped(x0, call, tape)
        else:
            if call.guard is not None:
                if self._range_record is None or self._range_record.device != dev:
                    self._range_record = torch.zeros(len(self._range_slot), dtype=torch.int32, device=dev)
                else:
                    self._range_record.zero_()
            x = self._forward_infer(x0, call)
            if call.guard == "fallback" and call.range_live:
                if max(self._range_record.tolist()) >= RANGE_OVER_BITS:      # one small copy + a synchronisation (|v|: sign bit clear)
                    self._range_tripped = True
                    call = call._replace(split=False, sp=False, range_live=False)
                    x = self._forward_infer(x0, call)
        self._last_call = call
        Hc, Wc = x.shape[2], x.shape[3]
        feat = torch.empty(V, B, self.fc_dim, dtype=torch.float32, device=dev)
        if x.dtype == torch.float16:                                # sp activation of the split path
            ops.avgpool_fwd_split(x, feat, V * B, Hc * Wc, self.fc_dim)
        else:
            ops.avgpool_fwd(x, feat, V * B, Hc * Wc, self.fc_dim)
        if keep_tape:
            tape["final_hw"] = (Hc, Wc)
        return feat, tape

    def _forward_infer(self, x0: Tensor, call: Call) -> Tensor:
        """Stem and residual blocks of the folded inference forward (see _unit_infer), in the order csrc/session_plan.cpp
        states (build for the fp32 model, build_bf16 for the bf16 path): conv1 up to the last conv, the downsample branch as a
        normalised residual, the last conv with residual + ReLU."""
        s = self.spec
        if call.bf16:         # the bf16 stem keeps the training-shaped launches: conv, then BatchNorm + ReLU + max pool in one pass
            x = self._unit_fwd(call, s.stem, x0, call.H, call.W, relu=True, pool=True).out
        else:
            x = self._unit_infer(call, s.stem, x0, call.H, call.W, True, None, pool=True)
        for blk in s.blocks:
            out = x
            for c in blk.convs[:-1]:
                out = self._unit_infer(call, c, out, out.shape[2], out.shape[3], True, None)
            identity = x
            if blk.downsample is not None:
                identity = self._unit_infer(call, blk.downsample, x, x.shape[2], x.shape[3], False, None)
            x = self._unit_infer(call, blk.convs[-1], out, out.shape[2], out.shape[3], True, identity)
        return x

    def _forward_taped(self, x0: Tensor, call: Call, tape: Optional[dict]) -> Tensor:
        """Stem and residual blocks through _unit_fwd: training, eval mode with a tape, and (tape None) unfolded bf16
        inference.  Fills tape["units"] / tape["blocks"]."""
        s = self.spec
        ulist = tape["units"] if tape is not None else None
        boundary = call.boundary
        x = self._unit_fwd(call, s.stem, x0, call.H, call.W, relu=True, tape=ulist, pool=True).out
        if boundary > -1:
            self._release(ulist[0])
        pending = None        # the previous block's apply pass, when this block's first conv forms its own input
        for bi, blk in enumerate(s.blocks):
            first = len(ulist) if ulist is not None else 0
            identity, ident_affine, ds_idx = x, None, None
            out = x
            for c in blk.convs[:-1]:
                # (conv1 runs before the downsample branch and before anything else that reads the block input)
                out = self._unit_fwd(call, c, out, out.shape[2], out.shape[3], relu=True, tape=ulist, pending_apply=pending).out
                pending = None
            if blk.downsample is not None:
                # raw downsample conv output + its (scale, shift): normalised inside the last unit's bn_apply
                identity, ident_affine, _ = self._unit_fwd(call, blk.downsample, x, x.shape[2], x.shape[3], relu=False, tape=ulist,
                                                           defer_apply=True)
                ds_idx = len(ulist) - 1 if ulist is not None else None
            nxt = s.blocks[bi + 1].convs[0] if (bi + 1 < len(s.blocks) and call.training and not call.bf16) else None
            x, _, pending = self._unit_fwd(call, blk.convs[-1], out, out.shape[2], out.shape[3], relu=True, residual=identity,
                                           tape=ulist, residual_affine=ident_affine, next_conv=nxt)
            if ulist is not None:
                tape["blocks"].append((list(range(first, first + len(blk.convs) - 1)) + [len(ulist) - 1], ds_idx))
                if bi < boundary:
                    for u in ulist[first:]:
                        self._release(u)
        return x

    def _boundary(self, need_dimg: bool) -> int:
        """Where back-propagation stops: the first unit in forward order - -1 for the stem, else the index of a residual block,
        its downsample unit counting with it - that owns a parameter with ``requires_grad``; len(blocks) when none does.
        Below it nothing is back-propagated (no BatchNorm backward, backward-data or weight-gradient launch, and the tape
        keeps none of those units' activations); the boundary block's own input gradient is not computed either.  A caller
        that wants d(loss)/d(img) back-propagates everything: -1."""
        s = self.spec

        def trainable(c: ConvSpec) -> bool:
            return any(getattr(self.p[n], "requires_grad", False) for n in (c.name + ".weight", c.bn + ".weight", c.bn + ".bias"))
        if need_dimg or trainable(s.stem):
            return -1
        for bi, blk in enumerate(s.blocks):
            if any(trainable(c) for c in list(blk.convs) + ([blk.downsample] if blk.downsample is not None else [])):
                return bi
        return len(s.blocks)

    @staticmethod
    def _release(u: _Unit) -> None:
        """A unit below the boundary: the tape keeps its place (the block records index into the list) and nothing else.  The
        forward launches were the same; what later units still read stays alive through their own x_in."""
        u.x_in = u.y = u.out = u.mean = u.invstd = u.w = u.pool = u.relu_affine = u.fused_s12 = u.relu_bits = None

    # ---------------------------------------------------------------- backward
    def _bn_params(self, c: ConvSpec, sink: GradSink):
        """(gamma, beta, accumulate): the BatchNorm parameters of unit ``c`` and whether their gradients are added to."""
        gp, bp = self.p[c.bn + ".weight"], self.p[c.bn + ".bias"]
        # (one flag serves both sums: a frozen one of the two follows the other - its slice of the arena is nobody's .grad)
        accs = {sink.accumulate(q) for q in (gp, bp) if sink.wants(q)}
        assert len(accs) <= 1
        return gp, bp, bool(accs) and accs.pop()

    def _unit_params(self, c: ConvSpec) -> List[torch.nn.Parameter]:
        """The parameters whose gradients are final once unit ``c``'s backward is queued (GradSink.publish)."""
        return [self.p[c.name + ".weight"], self.p[c.bn + ".weight"], self.p[c.bn + ".bias"]]

    def _bn_bwd(self, u: _Unit, g: Tensor, need_dz: bool, sink: GradSink, defer_apply: bool = False):
        """g = grad wrt the unit's output.  Returns (dy, dz, pending): dy = grad wrt the conv output;
        dz = g masked by the unit's ReLU (written in place into g) when the residual branch needs it.
        defer_apply (a unit that bn_apply_dgrad_eligible accepted): dy is only allocated - the unit's backward-data launch
        forms and writes it from ``pending`` (a _PendingDy; else None)."""
        if not u.trained and u.family is Family.SPLIT:
            return self._bn_bwd_frozen_split(u, g, need_dz, sink) + (None,)
        if not u.trained:
            return self._bn_bwd_eval(u, g, need_dz, sink) + (None,)
        c = u.spec
        G = u.y.shape[0]
        gp, bp, acc = self._bn_params(c, sink)
        fs, u.fused_s12 = u.fused_s12, None
        if u.family is Family.SPLIT:
            # g and y are fp32, dy goes to the conv kernels in sp
            dy = ops.sp_empty(*u.y.shape, device=g.device)
            if fs is not None:
                # fused: g arrived masked and the sums came with it
                if defer_apply:
                    dy.sinv = fs.sinv
                    return dy, (g if need_dz else None), _PendingDy(g, fs.s1, fs.s2)
                ops.bn_bwd_apply_split(g, u.y, u.mean, u.invstd, gp.detach(), fs.s1, fs.s2, G, u.rows, c.cout, dy, None, fs.mx, fs.sinv)
                return dy, (g if need_dz else None), None
            # residual units carry their mask as bits.  No pass here reads the (scaled) sp activation: the mask comes from
            # the bits or from fma(y, scale, shift) > 0, both decided on the unscaled value
            bits, ra = u.relu_bits, u.relu_affine
            assert not (u.relu and ra is None) or bits is not None
            s12 = torch.empty(3, G, c.cout, dtype=torch.float32, device=g.device)     # s1, s2, max |dz| per channel
            sinv = torch.empty(1, dtype=torch.float32, device=g.device)       # dy's 2^-k: left by the reduce pass's finalize launch
            ra = None if bits is not None else ra                 # one mask source; with bits the reduce pass leaves dz in g
            ops.bn_bwd_reduce_split(g, bits, u.y, u.mean, u.invstd, G, u.rows, c.cout, s12[0], s12[1], sink.view(gp), sink.view(bp),
                                    acc, s12[2], ra, dz_out=g if bits is not None else None, gamma=gp.detach(), dy_sinv=sinv)
            ops.bn_bwd_apply_split(g, u.y, u.mean, u.invstd, gp.detach(), s12[0], s12[1], G, u.rows, c.cout, dy, ra, s12[2], sinv)
            return dy, (g if need_dz else None), None
        # FP32 / BF16: the passes follow the storage type of g
        if fs is not None:
            # g arrived masked by this unit's ReLU and its sums (incl. dgamma / dbeta) came with it
            dy = torch.empty_like(g) if need_dz else g
            ops.bn_bwd_apply(g, None, u.y, u.mean, u.invstd, gp.detach(), fs.s1, fs.s2, G, u.rows, c.cout, dy, None, None)
            return dy, (g if need_dz else None), None
        s12 = torch.empty(2, G, c.cout, dtype=torch.float32, device=g.device)         # s1, s2
        ra = u.relu_affine
        act = u.out if (u.relu and ra is None) else None
        # need_dz: the reduce pass writes the masked gradient dz over g: the apply pass then reads (dz, y) only - no
        # second look at the ReLU mask, no second dz store - and the residual branch takes dz from g
        if need_dz and u.relu_bits is not None:
            ops.bn_bwd_reduce_bits(g, u.relu_bits, u.y, u.mean, u.invstd, G, u.rows, c.cout, s12[0], s12[1], sink.view(gp),
                                   sink.view(bp), acc, dz_out=g)
        else:
            ops.bn_bwd_reduce(g, act, u.y, u.mean, u.invstd, G, u.rows, c.cout, s12[0], s12[1], sink.view(gp), sink.view(bp),
                              acc, ra, dz_out=g if need_dz else None)
        if need_dz:
            dy = torch.empty_like(g)
            ops.bn_bwd_apply(g, None, u.y, u.mean, u.invstd, gp.detach(), s12[0], s12[1], G, u.rows, c.cout, dy, None, None)
            return dy, g, None
        ops.bn_bwd_apply(g, act, u.y, u.mean, u.invstd, gp.detach(), s12[0], s12[1], G, u.rows, c.cout, g, None, ra)
        return g, None, None

    def _bn_bwd_eval(self, u: _Unit, g: Tensor, need_dz: bool, sink: GradSink):
        """_bn_bwd for a unit whose forward normalised with the running statistics (eval mode, or a frozen-BatchNorm training
        step; fp32-MFMA or bf16 kernels - the pass follows the storage type of g): one pass (ops.bn_eval_bwd) - dy needs no
        batch sums.  The tape's mean / invstd were never filled and are not read: the kernel takes the running statistics, and
        the ReLU mask from where the forward left it."""
        c = u.spec
        G = u.y.shape[0]
        gp, bp, acc = self._bn_params(c, sink)
        rm, rv = self.p[c.bn + ".running_mean"], self.p[c.bn + ".running_var"]
        if u.relu_bits is not None:
            mask = {"relu_bits": u.relu_bits}
        elif u.relu_affine is not None:
            mask = {"relu_affine": u.relu_affine}
        elif u.relu:
            mask = {"act": u.out}
        else:
            mask = {}
        # the residual branch needs dz: it stays in g, dy goes to a new buffer; otherwise dy overwrites g
        dy = torch.empty_like(g) if need_dz else g
        ops.bn_eval_bwd(g, u.y, gp.detach(), rm, rv, BN_EPS, G, u.rows, c.cout, dy, sink.view(gp), sink.view(bp), acc,
                        dz_out=g if need_dz else None, **mask)
        return dy, (g if need_dz else None)

    def _bn_bwd_frozen_split(self, u: _Unit, g: Tensor, need_dz: bool, sink: GradSink):
        """_bn_bwd for a unit of a frozen-BatchNorm step on the split kernels: the reduce forms of a trained unit - fused into
        the backward-data launch that produced g, or the pass of its own - run on the tape's (mean, invstd), which hold the
        running values, so their s1 / s2 ARE dbeta / dgamma and their dy scale bounds the frozen dy; the apply pass is
        ops.bn_frozen_bwd_apply_split: dy = gamma invstd dz in sp, one pass, no sums."""
        c = u.spec
        G = u.y.shape[0]
        gp, bp, acc = self._bn_params(c, sink)
        fs, u.fused_s12 = u.fused_s12, None
        dy = ops.sp_empty(*u.y.shape, device=g.device)
        if fs is not None:                    # g arrived masked; dgamma, dbeta and the scale came with it
            ops.bn_frozen_bwd_apply_split(g, u.y, u.invstd, gp.detach(), G, u.rows, c.cout, dy, fs.sinv)
            return dy, (g if need_dz else None)
        bits, ra = u.relu_bits, u.relu_affine
        assert not (u.relu and ra is None) or bits is not None
        s12 = torch.empty(3, G, c.cout, dtype=torch.float32, device=g.device)     # s1, s2, max |dz| per channel
        sinv = torch.empty(1, dtype=torch.float32, device=g.device)
        ra = None if bits is not None else ra                 # one mask source; with bits the reduce pass leaves dz in g
        ops.bn_bwd_reduce_split(g, bits, u.y, u.mean, u.invstd, G, u.rows, c.cout, s12[0], s12[1], sink.view(gp), sink.view(bp),
                                acc, s12[2], ra, dz_out=g if bits is not None else None, gamma=gp.detach(), dy_sinv=sinv)
        ops.bn_frozen_bwd_apply_split(g, u.y, u.invstd, gp.detach(), G, u.rows, c.cout, dy, sinv, ra)
        return dy, (g if need_dz else None)

    def _side(self, dev) -> "torch.cuda.Stream":
        if self._wg_stream is None or self._wg_stream.device != dev or self._wg_low != self.wgrad_low_priority:
            old = self._wg_stream if (self._wg_stream is not None and self._wg_stream.device == dev) else None
            self._wg_low = self.wgrad_low_priority
            try:
                if not self._wg_low:
                    raise RuntimeError
                self._wg_stream = ops.low_priority_stream(dev)   # fills what the critical path leaves idle
            except RuntimeError:                                 # ordinary side stream (also: no priority support)
                self._wg_stream = torch.cuda.Stream(device=dev)
            if old is not None:
                self._wg_stream.wait_stream(old)                 # whoever joins the new stream also joins the old one's work
            self.grad_streams[:] = [self._wg_stream]
        return self._wg_stream

    def _conv_bwd(self, u: _Unit, dy: Tensor, need_dx: bool, addend: Optional[Tensor], sink: GradSink,
                  fuse_for: Optional[_Unit] = None, pending: Optional[_PendingDy] = None):
        """The weight gradient of unit u (on the side stream) and, with need_dx, its backward-data launch.  pending: dy does
        not exist yet - the backward-data launch forms it and writes it first, then the weight gradient reads it."""
        dx = None
        if pending is not None:
            dx = torch.empty(ops.sp_shape(u.x_in), dtype=torch.float32, device=dy.device)
            self._dgrad(u, dy, dx, addend, fuse_for, sink, pending)
            need_dx = False
        if not sink.wants(self.p[u.spec.name + ".weight"]):
            pass          # a frozen conv weight: no weight-gradient launch, no slabs for the block's deferred reduce
        elif self.overlap_wgrad and dy.is_cuda:
            side = self._side(dy.device)
            side.wait_stream(torch.cuda.current_stream())         # dy (and everything before it) is ready
            with torch.cuda.stream(side):
                self._wgrad(u, dy, sink)
            if getattr(dy, "sinv", None) is not None:
                dy.sinv.record_stream(side)
            dy.record_stream(side)                                # the allocator must not recycle these while
            u.x_in.record_stream(side)                            # the side stream still reads them
            if getattr(u.x_in, "sinv", None) is not None:         # (a scaled sp activation: its slot too)
                u.x_in.sinv.record_stream(side)
        else:
            self._wgrad(u, dy, sink)
        if need_dx:
            dx = (torch.empty(ops.sp_shape(u.x_in), dtype=torch.float32, device=dy.device) if u.family is Family.SPLIT
                  else torch.empty_like(u.x_in))
            self._dgrad(u, dy, dx, addend, fuse_for, sink)
        return dx

    def _wgrad(self, u: _Unit, dy: Tensor, sink: GradSink):
        c = u.spec
        wp = self.p[c.name + ".weight"]
        if u.family is Family.SPLIT:
            if u.stem_rw:
                dw8 = torch.empty(c.cout, 7, 8, 4, dtype=torch.float32, device=dy.device)
                ops.stem_wgrad_split(u.desc, u.x_in, dy, dw8, False)
                self._stem_grad(wp, sink, dw8[:, :, 1:, :3])
            else:
                # (slabs now, their sums in ONE launch per residual block: _flush_wgrad_reduces); x_in is read by VALUE: its
                # .sinv goes into the launch's output scale
                ops.conv_wgrad_split(u.desc, u.x_in, dy, sink.view(wp), sink.accumulate(wp), defer=self._wg_defer)
        elif u.stem_rw:                      # (BF16: the folded windows)
            dw16 = torch.empty(2 * c.cout, 7, 16, 4, dtype=torch.float32, device=dy.device)
            ops.stem_wgrad_bf16(u.desc, u.x_in, dy, dw16, False)
            self._stem_grad(wp, sink, dw16[:c.cout, :, 1:8, :3], dw16[c.cout:, :, 3:10, :3])    # (second: the odd output columns' taps)
        elif c.cin == 3:                     # (FP32 / BF16: the stem on taps padded to 4 / 8 channels)
            dw4 = torch.empty(c.cout, c.k, c.k, u.desc.cin, dtype=torch.float32, device=dy.device)
            ops.conv_wgrad(u.desc, u.x_in, dy, dw4, False)
            self._stem_grad(wp, sink, dw4[..., :3])
        else:
            ops.conv_wgrad(u.desc, u.x_in, dy, sink.view(wp), sink.accumulate(wp),
                           defer=self._wg_defer if u.family is Family.BF16 else None)

    @staticmethod
    def _stem_grad(wp: torch.nn.Parameter, sink: GradSink, dw: Tensor, dw_odd: Optional[Tensor] = None):
        """The stem's weight gradient, computed into a padded buffer, into the parameter's gradient: ``dw`` (and ``dw_odd``,
        the second filter copy of the bf16 two-parity form) are [cout, 7, 7, 3] slices of that buffer."""
        gv = sink.view(wp).permute(0, 2, 3, 1)                        # [cout, 7, 7, 3] view of the gradient
        if sink.accumulate(wp):
            gv.add_(dw)
        else:
            gv.copy_(dw)
        if dw_odd is not None:
            gv.add_(dw_odd)

    def _flush_wgrad_reduces(self, dev):
        """The slab sums of the weight gradients launched since the last flush, in one launch on the stream that wrote the slabs."""
        if not self._wg_defer:
            return
        if self.overlap_wgrad and dev.type == "cuda":
            with torch.cuda.stream(self._side(dev)):
                ops.wgrad_reduce_batch(self._wg_defer)
        else:
            ops.wgrad_reduce_batch(self._wg_defer)

    def _dgrad(self, u: _Unit, dy: Tensor, dx: Tensor, addend: Optional[Tensor], fuse_for: Optional[_Unit] = None,
               sink: Optional[GradSink] = None, pending: Optional[_PendingDy] = None):
        """dx = backward-data of unit u (+ addend).  fuse_for = the unit whose OUTPUT gradient dx is, when dx
        is final with this launch: its ReLU mask is applied and its BatchNorm-backward sums (s1, s2, dgamma,
        dbeta) are produced by the same launch (mvg_conv_dgrad_split_bnreduce / mvg_conv_dgrad_bf16_bnreduce; stride-2 launches
        too: every parity class brings its partials) instead of a pass over (g, act, y).  pending: the launch forms dy too."""
        U = fuse_for if self.fuse_bn_split else None
        if u.family is Family.BF16:
            # (a unit on running statistics has no mean / invstd and its one-pass backward needs no batch sums: plain launch)
            if (U is not None and U.trained and u.spec.cin != 3 and u.desc.cin % 64 == 0 and u.desc.cout % 64 == 0
                    and (not U.relu or U.relu_bits is not None or U.relu_affine is not None)):     # (relu_bits off: mask from the activation)
                c = U.spec
                gp, bp, acc = self._bn_params(c, sink)
                s12 = torch.empty(2, dx.shape[0], c.cout, dtype=torch.float32, device=dx.device)
                ops.conv_dgrad_bf16_bnreduce(u.desc, dy, u.w, dx, addend, U.y, U.relu_bits, U.mean, U.invstd,
                                             None if U.relu_bits is not None else U.relu_affine, s12[0], s12[1], sink.view(gp),
                                             sink.view(bp), acc)
                U.fused_s12 = _FusedSums(s12[0], s12[1])
            else:
                ops.conv_dgrad(u.desc, dy, u.w, dx, None, addend)
        elif u.family is Family.SPLIT:
            if U is not None and U.family is Family.SPLIT:
                c = U.spec
                gp, bp, acc = self._bn_params(c, sink)
                # (the fused reduce epilogue masks with U's bits or fma(U.y, scale, shift) > 0: no sp activation is read)
                s12 = torch.empty(3, dx.shape[0], c.cout, dtype=torch.float32, device=dx.device)     # s1, s2, max |dz| per channel
                sinv = torch.empty(1, dtype=torch.float32, device=dx.device)      # 2^-k of the dy that U's apply pass will write
                ra = None if U.relu_bits is not None else U.relu_affine
                if pending is not None:
                    p, ugamma = pending, self.p[u.spec.bn + ".weight"].detach()
                    ops.conv_dgrad_split_bnapply_bnreduce(u.desc, dy, dy.sinv, p.dz, u.y, u.mean, u.invstd, ugamma, p.s1, p.s2, u.rows,
                                                          u.w, dx, addend, U.y, U.relu_bits, U.mean, U.invstd, ra, s12[0], s12[1],
                                                          sink.view(gp), sink.view(bp), acc, s12[2], gp.detach(), sinv)
                else:
                    ops.conv_dgrad_split_bnreduce(u.desc, dy, u.w, dx, addend, U.y, U.relu_bits, U.mean, U.invstd, ra, s12[0], s12[1],
                                                  sink.view(gp), sink.view(bp), acc, s12[2], gp.detach(), sinv)
                U.fused_s12 = _FusedSums(s12[0], s12[1], s12[2], sinv)
            else:
                assert pending is None       # (bn_apply_dgrad_eligible: the launch that forms dy carries a reduce)
                ops.conv_dgrad_split(u.desc, dy, u.w, dx, addend)
        else:
            ops.conv_dgrad(u.desc, dy, u.w, dx, None, addend)

    def _stem_bn_bwd(self, stem: _Unit, g: Tensor, V: int, B: int, sink: GradSink) -> Tensor:
        """The stem's max pool + ReLU + BatchNorm backward, fused (the 112x112 gradient map is never built): g = grad wrt
        the pooled map; returns dy = grad wrt the stem conv's output."""
        argmax, scale, shift, H1, W1, Hp, Wp = stem.pool
        sc = stem.spec
        P = self.p
        gp, bp, acc = self._bn_params(sc, sink)
        stem_sp = stem.family is Family.SPLIT       # (the row-window stem of a split call)
        s12 = torch.empty(3 if stem_sp else 2, V, sc.cout, dtype=torch.float32, device=g.device)
        if not stem.trained and stem_sp:
            # a frozen step with the row-window stem (once per step: no form of its own): the train-mode pair on the running
            # (mean, invstd) the tape holds - the reduce pass leaves dbeta, dgamma and a dy scale whose bound only gains
            # non-negative terms from the sums - and the apply pass with ZERO sums: dy = gamma invstd dz exactly
            sinv = torch.empty(1, dtype=torch.float32, device=g.device)
            ops.bn_relu_maxpool_bwd_reduce_split(g, argmax, stem.y, stem.mean, stem.invstd, scale, shift, V, B, H1, W1, sc.cout, Hp, Wp,
                                                 s12[0], s12[1], sink.view(gp), sink.view(bp), acc, s12[2], gp.detach(), sinv)
            zero = torch.zeros(2, V, sc.cout, dtype=torch.float32, device=g.device)
            dy = ops.sp_empty(*stem.y.shape, device=g.device)
            ops.bn_relu_maxpool_bwd_apply_split(g, argmax, stem.y, stem.mean, stem.invstd, gp.detach(), scale, shift, zero[0], zero[1],
                                                V, B, H1, W1, sc.cout, Hp, Wp, dy, s12[2], sinv)
        elif not stem.trained:
            # eval mode: max pool + ReLU + BatchNorm on the running statistics, one pass (no batch sums to wait for)
            dy = torch.empty_like(stem.y)
            ops.bn_relu_maxpool_eval_bwd(g, argmax, stem.y, scale, shift, gp.detach(), P[sc.bn + ".running_mean"],
                                         P[sc.bn + ".running_var"], BN_EPS, V, B, H1, W1, sc.cout, Hp, Wp, dy, sink.view(gp),
                                         sink.view(bp), acc)
        elif stem_sp:
            # the stem's weight gradient runs on the split kernels: dy goes out in sp, scaled by a bound from the reduce pass
            sinv = torch.empty(1, dtype=torch.float32, device=g.device)
            ops.bn_relu_maxpool_bwd_reduce_split(g, argmax, stem.y, stem.mean, stem.invstd, scale, shift, V, B, H1, W1, sc.cout, Hp, Wp,
                                                 s12[0], s12[1], sink.view(gp), sink.view(bp), acc, s12[2], gp.detach(), sinv)
            dy = ops.sp_empty(*stem.y.shape, device=g.device)
            ops.bn_relu_maxpool_bwd_apply_split(g, argmax, stem.y, stem.mean, stem.invstd, gp.detach(), scale, shift, s12[0], s12[1],
                                                V, B, H1, W1, sc.cout, Hp, Wp, dy, s12[2], sinv)
        else:
            ops.bn_relu_maxpool_bwd_reduce(g, argmax, stem.y, stem.mean, stem.invstd, scale, shift, V, B, H1, W1, sc.cout, Hp, Wp,
                                           s12[0], s12[1], sink.view(gp), sink.view(bp), acc)
            dy = torch.empty_like(stem.y)
            ops.bn_relu_maxpool_bwd_apply(g, argmax, stem.y, stem.mean, stem.invstd, gp.detach(), scale, shift, s12[0], s12[1],
                                          V, B, H1, W1, sc.cout, Hp, Wp, dy)
        return dy

    def backward(self, tape: dict, dfeat: Tensor, sink: GradSink, need_dimg: bool = False):
        """dfeat [V,B,fc_dim] -> parameter gradients into ``sink`` (published layer4 ... stem, the
        order they become final); returns d(img) as V NCHW tensors when need_dimg."""
        call: Call = tape["call"]              # what the forward that wrote this tape ran on
        V, B = call.V, call.B
        units: List[_Unit] = tape["units"]
        if self.bf16 and not call.train_step and not all(u.trained for u in units):
            raise NotImplementedError("backward through eval-mode BatchNorm (running statistics) is not implemented on the "
                                      "bf16 path outside a training step: call model.train() - with model.freeze_batchnorm "
                                      "to keep the running statistics - for gradient steps, or use the fp32 model")
        Hc, Wc = tape["final_hw"]
        if need_dimg and self.bf16:
            raise NotImplementedError("d(loss)/d(img) is not produced by the bf16 path")
        if tape.get("wprep_versions") is not None and tape["wprep_versions"] != self._wprep_versions:
            raise RuntimeError("backward of a tape whose bf16 / sp weight copies were overwritten by a later forward with "
                               "DIFFERENT weights (forward, optimizer step, forward, then backward of the first call): "
                               "backward-data would run with the new weights.  Run backward before the weights change "
                               "(PyTorch raises its version-counter error in the same situation)")
        g = torch.empty(V, B, Hc, Wc, self.fc_dim, dtype=self.act_dtype, device=dfeat.device)
        ops.avgpool_bwd(dfeat.contiguous(), g, V * B, Hc * Wc, self.fc_dim)
        self._wg_defer = []
        blocks = tape["blocks"]
        # fine-tuning (see _boundary): back-propagation ends with the boundary block, whose input gradient nobody reads
        boundary = call.boundary
        assert not (need_dimg and boundary > -1), "the forward was not told that d(loss)/d(img) is wanted"
        for bi in range(len(blocks) - 1, max(boundary, 0) - 1, -1):
            idx, ds_idx = blocks[bi]
            need_in = bi > boundary               # False: the boundary block - no gradient leaves it
            last = units[idx[-1]]
            # the unit that receives this block's input gradient: the previous block's last unit (the stem's
            # fused pool backward takes it for the first block)
            prev_last = units[blocks[bi - 1][0][-1]] if bi > 0 else None
            done: List[torch.nn.Parameter] = []
            below = units[idx[-2]]
            merge = self.fuse_bn_apply_dgrad and bn_apply_dgrad_eligible(
                last.spec, split=last.family is Family.SPLIT, trained=last.trained, fused_in=last.fused_s12 is not None,
                carries_reduce=below.family is Family.SPLIT and self.fuse_bn_split, need_dimg=need_dimg)
            dy, dz, pending = self._bn_bwd(last, g, True, sink, defer_apply=merge)
            d = self._conv_bwd(last, dy, True, None, sink, fuse_for=below, pending=pending)
            done += self._unit_params(last.spec)
            last.y = last.out = None
            del dy
            for k in range(len(idx) - 2, -1, -1):
                u = units[idx[k]]
                dy = self._bn_bwd(u, d, False, sink)[0]
                if k == 0 and not need_in:
                    d = self._conv_bwd(u, dy, False, None, sink)              # the weight gradient only
                elif k == 0:
                    # with a downsample branch the block-input gradient is final only after that branch's launch
                    d = self._conv_bwd(u, dy, True, dz if ds_idx is None else None, sink,
                                       fuse_for=prev_last if ds_idx is None else None)
                else:
                    d = self._conv_bwd(u, dy, True, None, sink, fuse_for=units[idx[k - 1]])
                done += self._unit_params(u.spec)
                u.y = u.out = None
            if ds_idx is not None:
                ud = units[ds_idx]
                dyd = self._bn_bwd(ud, dz, False, sink)[0]
                self._conv_bwd(ud, dyd, False, None, sink)                # wgrad only
                if need_in:
                    self._dgrad(ud, dyd, d, d, prev_last, sink)           # d += dgrad (aliasing addend): now final
                done += self._unit_params(ud.spec)
                ud.y = ud.out = None
            self._flush_wgrad_reduces(g.device)               # this block's weight gradients are final once their slabs are summed
            sink.publish(done)
            g = d
            if "debug" in tape and g is not None:
                tape["debug"].append(g.clone())
        dx0 = None
        if boundary < 0:
            stem = units[0]
            dy = self._stem_bn_bwd(stem, g, V, B, sink)
            dx0 = self._conv_bwd(stem, dy, need_dimg, None, sink)
            self._flush_wgrad_reduces(dfeat.device)
            sink.publish(self._unit_params(stem.spec))
        self._wg_defer = None
        if self._wg_stream is not None and dfeat.is_cuda and (self.overlap_wgrad or not torch.cuda.is_current_stream_capturing()):
            torch.cuda.current_stream().wait_stream(self._wg_stream)      # gradients complete for the optimizer
        if not need_dimg:
            return None
        H, W = dx0.shape[2], dx0.shape[3]
        outs = []
        for v in range(V):
            o = torch.empty(B, 3, H, W, dtype=torch.float32, device=dx0.device)
            ops.nhwc4_to_nchw(dx0[v], o, B, 3, H, W)
            outs.append(o)
        return outs
