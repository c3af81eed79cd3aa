"""The launch trace of FusionHead.forward / FusionHead.backward, case by case, against a recorded golden file (the head's
counterpart of tests/test_backbone_trace_gpu.py; the recording rules are tests/launch_trace.py's).

tests/golden/head_launch_traces.txt is rewritten by
    python tests/test_head_trace_gpu.py --write
and  --dump DIR  writes the full traces, one file per case.  A refactor of heads.py keeps the file as the commit before it
wrote it: the sequence of launches, their arguments and their streams stay.

The head runs alone on ResNet-18 widths (cf = 512, fuser input 2048 wide).  The module goes only through model._head and its
four knobs (split, mixed, fused_input, keep_infer_copies), forward(img_feat, rot, keep_tape, training),
backward(tape, d_lifted, d_feats, d_preds, sink, side), model._sink and tape["mode"], so it runs on any commit that has them.
The split Linears need D * B >= 1024 rows: V = 2, B = 512 and V = 3, B = 171 (1026 rows) are the smallest such shapes;
everything else runs at B <= 4.  CASES and run_case are shared with scripts/step_digest.py (the same cases, hashed by value)."""
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import rot_mvgaze_amd  # noqa: F401,E402
from rot_mvgaze_amd import ops  # noqa: E402

import fusion_head_harness as H  # noqa: E402
import launch_trace as LT  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_launch_traces.txt")
TOOL = "test_head_trace_gpu.py"
BIG = dict(V=2, B=512)                       # 1024 rows: the row edge of the split Linears

# name -> shape, iteration count, variant, knobs of model._head, the tape mode the forward must report, and how the case runs:
#   (no "steps")  fusion_head_harness.run_head: one taped training forward, backward from d_preds
#   steps         a list run in order on one head: ("infer",) a tape-less eval forward; ("train", which, side) a taped training
#                 forward and its backward from the upstream gradients named in `which` ("l" d_lifted, "f" d_feats, "p" d_preds),
#                 weight gradients on a side stream if `side`
CASES = {
    "a_fp32_gen_V2_I3": dict(V=2, B=3, I=3, mode="fp32"),
    "b_fp32_materialised_V2_I3": dict(V=2, B=3, I=3, mode="fp32", knobs=dict(fused_input=False), steps=[("train", "p", False)]),
    "c_split_V2_B512_I3": dict(**BIG, I=3, mode="split"),
    "d_split_V3_B171_I2": dict(V=3, B=171, I=2, mode="split"),
    "e_split_asked_I6_runs_fp32": dict(**BIG, I=6, mode="fp32"),
    "f_split_share_weights": dict(**BIG, I=3, mode="split", variant=dict(share_weights=True)),
    "g_split_ignore_rotmat": dict(**BIG, I=3, mode="split", variant=dict(ignore_rotmat=True)),
    "h_mixed_I3": dict(V=2, B=3, I=3, mode="mixed", split=False, mixed=True),
    "i_encode_rotmat_V3": dict(V=3, B=2, I=3, mode="fp32", variant=dict(encode_rotmat=True)),
    "j_share_feature_train": dict(V=2, B=4, I=3, mode="fp32", variant=dict(share_feature=True)),
    "k_mixed_infer_twice_reuses_copies": dict(V=2, B=3, I=3, split=False, mixed=True, steps=[("infer",), ("infer",)]),
    "l_mixed_infer_twice_no_keep": dict(V=2, B=3, I=3, split=False, mixed=True, knobs=dict(keep_infer_copies=False),
                                        steps=[("infer",), ("infer",)]),
    "m_fp32_partial_grads": dict(V=2, B=3, I=3, mode="fp32", steps=[("train", w, False) for w in ("p", "f", "l")]),
    "m_split_partial_grads": dict(**BIG, I=3, mode="split", steps=[("train", w, False) for w in ("p", "f", "l")]),
    "n_fp32_side_stream": dict(V=2, B=3, I=3, mode="fp32", steps=[("train", "lfp", True)]),
    "n_split_side_stream": dict(**BIG, I=3, mode="split", steps=[("train", "lfp", True)]),
    # forward A (split, taped), forward B (small, fp32: muted in the trace), backward of A
    "o_split_tape_survives_other_forward": dict(**BIG, I=3, mode="split", steps=[("train", "p", False)], between=dict(V=2, B=2, mode="fp32")),
}


def _build(cfg):
    """The model run_head builds (synth weights, training mode, laid out on the device), its head with the case's knobs set."""
    from rot_mvgaze_amd import synth
    from rot_mvgaze_amd.arch import Variant
    from rot_mvgaze_amd.model import MultiViewGaze
    I, variant = cfg["I"], Variant(**cfg["variant"]) if cfg.get("variant") else None
    raw = synth.make_state_dict(18, 0, I, variant=variant) if variant is not None else synth.make_state_dict(18, 0, I)
    m = MultiViewGaze(18, I, variant) if variant is not None else MultiViewGaze(18, I)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in raw.items()}, strict=True)
    m.to(H.dev()).train()
    m.ensure_layout()
    return m


def _inputs(m, V, B, seed):
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    torch.manual_seed(seed)
    img_feat = (torch.rand(V, B, m._fc_dim, device=H.dev()) * 2.0).contiguous()
    rot = rotation_matrix_2d(torch.rand(B * V, 2, device=H.dev()) - 0.5).reshape(B, V, 3, 3)
    return img_feat, rot


def _backward(m, tape, d_lifted, d_feats, d_preds, side):
    for p in m.parameters():
        p.grad = None
    m._sink.active = False
    m._sink.begin()
    dimg = m._head.backward(tape, d_lifted, d_feats, d_preds, m._sink, side)
    m._sink.active = False
    return dimg


def run_case(name):
    """Run the case.  Returns (model, results): per step a dict of the tensors it produced (feats, preds, dimg where there are)."""
    cfg = CASES[name]
    V, B, I = cfg["V"], cfg["B"], cfg["I"]
    ops.set_reserved_cus(0)                  # the planners see the whole device, whatever ran before
    if "steps" not in cfg:
        assert not cfg.get("knobs")
        run = H.run_head(18, V, B, I, variant_kw=cfg.get("variant"), split=cfg.get("split", True), mixed=cfg.get("mixed", False))
        assert run["tape"]["mode"] == cfg["mode"], run["tape"]["mode"]
        return run["m"], [dict(feats=run["feats"], preds=run["preds"], dimg=run["dimg"])]
    m = _build(cfg)
    head = m._head
    head.split, head.mixed = cfg.get("split", True), cfg.get("mixed", False)
    for k, v in cfg.get("knobs", {}).items():
        assert hasattr(head, k), k
        setattr(head, k, v)
    side = torch.cuda.Stream() if any(s[0] == "train" and s[2] for s in cfg["steps"]) else None
    results = []
    for n, step in enumerate(cfg["steps"]):
        img_feat, rot = _inputs(m, V, B, 5 + n)
        if step[0] == "infer":
            with torch.no_grad():
                lifted, feats, preds, tape = head.forward(img_feat, rot, False, False)
            assert tape is None
            results.append(dict(lifted=lifted, feats=feats, preds=preds))
            continue
        _, which, use_side = step
        lifted, feats, preds, tape = head.forward(img_feat, rot, True, True)
        assert tape["mode"] == cfg["mode"], tape["mode"]
        if "between" in cfg:                 # another forward, at another family, before the tape is used
            bt = cfg["between"]
            with LT.muted():
                out_b = head.forward(*_inputs(m, bt["V"], bt["B"], 99), True, True)
            assert out_b[3]["mode"] == bt["mode"] != tape["mode"]
        d_lifted = torch.randn_like(lifted) if "l" in which else None
        d_feats = torch.randn_like(feats) if "f" in which else None
        d_preds = torch.randn_like(preds) if "p" in which else None
        dimg = _backward(m, tape, d_lifted, d_feats, d_preds, side if use_side else None)
        results.append(dict(feats=feats, preds=preds, dimg=dimg))
    torch.cuda.synchronize()
    return m, results


def trace_case(name):
    from rot_mvgaze_amd.heads import FusionHead
    return LT.record(FusionHead, ("forward", "backward"), lambda: run_case(name))[0]


def _calls(lines, entry):
    return sum(l.split(" ", 1)[0] == entry for l in lines)


@pytest.mark.parametrize("name", sorted(CASES))
def test_launch_trace_is_the_recorded_one(name):
    lines = trace_case(name)
    assert _calls(lines, "mvg_cast_weights_bf16") == 0              # the bf16 copies come from the one batched launch only
    if name.startswith(("c_", "d_", "f_", "g_")):                   # the split Linears are reached at these rows (the lifter: fp32)
        assert _calls(lines, "mvg_linear_fprop_split") == 3 * CASES[name]["I"] and _calls(lines, "mvg_linear_fprop") == 2
    if name.startswith("e_"):
        assert _calls(lines, "mvg_linear_fprop_split") == 0 and _calls(lines, "mvg_fuser_fprop") == 12
    if name.startswith("k_"):                                       # the second call casts nothing
        assert _calls(lines, "mvg_weights_prep_batch") == 1
    if name.startswith("l_"):
        assert _calls(lines, "mvg_weights_prep_batch") == 2
    if name.startswith("n_"):                                       # the weight gradients went to the side stream
        assert any(l.endswith(" stream1") for l in lines) and lines[0].endswith(" stream0")
    if name.startswith("o_"):                                       # the tape carries what its backward needs
        alone = dict(CASES[name])
        del alone["between"]
        CASES["_o_alone"] = alone
        try:
            assert lines == trace_case("_o_alone")
        finally:
            del CASES["_o_alone"]
    LT.assert_matches_golden(name, lines, LT.read_golden(GOLDEN_FILE), TOOL)


if __name__ == "__main__":
    LT.write_or_dump(sys.argv[1:], sorted(CASES), trace_case, GOLDEN_FILE, TOOL)
