"""The launch trace of Backbone.forward / Backbone.backward, case by case, against a recorded golden file.

What a case records: every C call of the package made while Backbone.forward or Backbone.backward is on the stack (ops.lib is
replaced by a proxy; the two methods are wrapped to switch the recording) - the entry point's name, the fields of a ConvDesc
argument, every integer and float argument, whether each pointer argument is null (by the argument types of _lib.SIGNATURES),
and the stream the call is queued on as an ordinal by first appearance.  Pointer VALUES are not recorded: addresses depend on
allocation order, which may change.  mvg_set_scratch / mvg_scratch_bytes are left out: whether a stream's workspace is
already registered depends on what ran earlier in the process.  (The recorder is tests/launch_trace.py, shared with
tests/test_head_trace_gpu.py.)

tests/golden/backbone_launch_traces.txt holds, per case, a sha256 of the trace, the number of calls and the count per entry
point; on a mismatch the test says which counts moved.  The file is rewritten by
    python tests/test_backbone_trace_gpu.py --write
and  --dump DIR  writes the full traces, one file per case, so that two commits can be diffed.  A refactor of backbone.py
keeps the file as the commit before it wrote it: the sequence of launches, their arguments and their streams stay.

The module goes through the model's public surface only (attributes of the model and of model._backbone), so it runs on any
commit that has them.  CASES and run_case are shared with scripts/step_digest.py (the same cases, hashed by value)."""
import os
import random
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import rot_mvgaze_amd  # noqa: F401,E402
from rot_mvgaze_amd import ops, synth  # noqa: E402

import launch_trace as LT  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "backbone_launch_traces.txt")
BB = "_feat_extractor.0."
ALL_FUSIONS_OFF = dict(fuse_bn_split=False, fuse_bn_apply_dgrad=False, fuse_bn_apply_fprop=False, relu_bits=False, overlap_wgrad=False)

# name -> how the case is run (run_case): V = 2, B = 2 throughout; 64 x 64 unless hw says otherwise.
#   mode: "train" (a training step: forward, loss, backward), "eval_tape" (eval mode with gradients), "infer" (no_grad)
#   bb: attributes of model._backbone; model: attributes of the model; freeze: parameter-name prefixes below BB
#   raw: uint8 patches of that size (input_size: the model's resize target); augment: a seeded TrainAugment
CASES = {
    "01_r50_fp32_train": dict(depth=50),
    "02_r18_fp32_train": dict(depth=18),
    "03_r50_fp32_train_unfused": dict(depth=50, bb=ALL_FUSIONS_OFF),
    "04_r50_fp32_train_dimg": dict(depth=50, img_grad=True),
    "05_r18_fp32mfma_train": dict(depth=18, bb=dict(split=False)),
    "06_r50_bf16_train": dict(depth=50, bf16=True),
    "07_r50_bf16_train_72": dict(depth=50, bf16=True, hw=72),
    "08_r50_bf16_train_unfused": dict(depth=50, bf16=True, bb=dict(fuse_bn_split=False, relu_bits=False)),
    "09_r50_fp32_eval_tape": dict(depth=50, mode="eval_tape"),
    "10_r50_fp32_finetune": dict(depth=50, freeze=("conv1.", "bn1.", "layer1.")),
    "11_r50_fp32_infer_record": dict(depth=50, mode="infer", model=dict(split_eval_guard="record")),
    "12_r50_fp32_infer_fp32mfma": dict(depth=50, mode="infer", bb=dict(split_eval=False)),
    "13_r50_bf16_infer": dict(depth=50, mode="infer", bf16=True),
    "14_r50_bf16_infer_unfolded": dict(depth=50, mode="infer", bf16=True, bb=dict(bf16_fold_eval=False)),
    "15a_r18_fp32_infer_raw_resize": dict(depth=18, mode="infer", raw=48, model=dict(input_size=64)),
    "15b_r18_fp32_train_raw_augment": dict(depth=18, raw=64, augment=True, model=dict(input_size=None, input_bgr=True)),
}


def dev():
    return torch.device("cuda:0")


_SD = {}


def _state_dict(depth):
    if depth not in _SD:
        sd = synth.make_state_dict(depth, 0, 3, perturb_bn=True)
        _SD[depth] = {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}
    return _SD[depth]


def run_case(name):
    """Build the case's model and run its one step.  Returns (model, data, loss or None): data is the model's output dict."""
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    from rot_mvgaze_amd.losses import IterationLoss, StereoL1Loss
    from rot_mvgaze_amd.model import FeatRotationSymm
    cfg = CASES[name]
    depth, hw, mode, B = cfg["depth"], cfg.get("hw", 64), cfg.get("mode", "train"), 2
    ops.set_reserved_cus(0)                  # the planners see the whole device, whatever ran before
    torch.manual_seed(77), random.seed(77), np.random.seed(77)
    m = FeatRotationSymm(backbone_depth=depth, num_iter=3)
    m.load_state_dict(_state_dict(depth), strict=True)
    m.to(dev())
    m = m.train() if mode == "train" else m.eval()
    if cfg.get("bf16"):
        m.compute_dtype = torch.bfloat16
    m._ensure_layout(dev())
    for k, v in cfg.get("bb", {}).items():
        assert hasattr(m._backbone, k), k
        setattr(m._backbone, k, v)
    for k, v in cfg.get("model", {}).items():
        assert hasattr(m, k), k
        setattr(m, k, v)
    if cfg.get("augment"):
        from rot_mvgaze_amd.augment import TrainAugment
        m.input_augment = TrainAugment()
    frozen = cfg.get("freeze", ())
    for k, p in m.named_parameters():
        if any(k.startswith(BB + f) for f in frozen):
            p.requires_grad_(False)
    inp = synth.make_inputs(B, 2, 1234, hw)
    hp, gt = (torch.from_numpy(inp[k]).to(dev()) for k in ("head_pose", "gt_gaze"))
    if cfg.get("raw"):
        rng = np.random.RandomState(5)
        imgs = [torch.from_numpy(rng.randint(0, 256, (B, cfg["raw"], cfg["raw"], 3)).astype(np.uint8)).to(dev()) for _ in range(2)]
    else:
        img = torch.from_numpy(inp["img"]).to(dev())
        imgs = [img[:, v].contiguous().requires_grad_(bool(cfg.get("img_grad"))) for v in range(2)]
    data = {"img_0": imgs[0], "img_1": imgs[1],
            "rot_0": rotation_matrix_2d(hp[:, 0].contiguous()), "rot_1": rotation_matrix_2d(hp[:, 1].contiguous()),
            "gt_gaze": gt[:, 0].contiguous(), "gt_gaze_1": gt[:, 1].contiguous()}
    if mode == "infer":
        with torch.no_grad():
            out = m(data)
        torch.cuda.synchronize()
        return m, out, None
    out = m(data)
    loss = IterationLoss(StereoL1Loss(rel_weight=0.01, reference_decay=1.0), iter_decay=0.5)(out)
    loss.backward()
    torch.cuda.synchronize()
    return m, out, loss


def trace_case(name):
    """The trace lines of one case, and whether its stem ran in row-window form."""
    from rot_mvgaze_amd.backbone import Backbone
    lines, (m, out, loss) = LT.record(Backbone, ("forward", "backward"), lambda: run_case(name))
    return lines, bool(m._backbone._stem_rw)


@pytest.mark.parametrize("name", sorted(CASES))
def test_launch_trace_is_the_recorded_one(name):
    lines, stem_rw = trace_case(name)
    digest, n, counts = LT.summarise(lines)
    if name == "01_r50_fp32_train":          # the loader-formed launches are reached at this size
        assert counts.get("mvg_conv_fprop_split_bnapply", 0) >= 1 and counts.get("mvg_conv_dgrad_split_bnapply_bnreduce", 0) >= 1, counts
    if name == "07_r50_bf16_train_72":       # 2 * 36 * 18 partial rows: no multiple of 64, the NHWC8 stem
        assert stem_rw is False
    LT.assert_matches_golden(name, lines, LT.read_golden(GOLDEN_FILE), "test_backbone_trace_gpu.py")


def main(argv):
    LT.write_or_dump(argv, sorted(CASES), lambda name: trace_case(name)[0], GOLDEN_FILE, "test_backbone_trace_gpu.py")


if __name__ == "__main__":
    main(sys.argv[1:])
