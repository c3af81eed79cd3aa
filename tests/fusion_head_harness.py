"""The fusion head alone against the fp64 oracle of the same block, for any iteration count (shared by
tests/test_fusion_split_gpu.py, which runs it at 3, and tests/test_iter_count_gpu.py).

head.forward(img_feat, rot, True, True) on random pooled features, head.backward for a random upstream gradient on the
predictions, then oracle/restatement.py's lift / fuse_pair on the same features in float64 with the HIP forward's ReLU
patterns IMPOSED (oracle/restatement.py:_relu): a hidden unit within fp32 rounding of 0 may fall on either side, which moves
gradients discontinuously and says nothing about the kernels (first run of the split test without it: every output at 2e-5,
one weight gradient at 7e-4 from such flips).  Features, predictions, d / d img_feat and every parameter gradient of every
iteration are compared; with share_weights one device Parameter stands under several state_dict names and the oracle's
gradient is the sum over the names."""
import os

import numpy as np
import torch


def dev():
    return torch.device("cuda:0")


def rel_l2(a, ref):
    return ((a.double() - ref).norm() / ref.norm()).item()


def rel_max(a, ref):
    return ((a.double() - ref).abs().max() / ref.abs().max()).item()


METRICS = {"rel-L2": rel_l2, "max-norm": rel_max}


class Figures:
    """Every comparison's figure by group; `line(group)` prints smallest .. largest before the caller asserts."""

    def __init__(self, tag):
        self.tag, self.groups = tag, {}

    def add(self, group, err, what):
        self.groups.setdefault(group, []).append((err, what))

    def worst(self, group):
        return max(self.groups[group])

    def report(self, group, metric, bar):
        v = sorted(self.groups[group])
        line = (f"ITER-COUNT {self.tag} {group}: {metric} {v[0][0]:.3e} .. {v[-1][0]:.3e} over {len(v)} comparisons "
                f"(largest at {v[-1][1]}; bar {bar:.1e})")
        print(line)
        return line


def run_head(depth, V, B, I, variant_kw=None, fuser_scale=1.0, seed=5, split=True, mixed=False):
    """Build MultiViewGaze(depth, I[, variant]) from synth weights (every `_img_fusers.*` tensor times fuser_scale), run the
    head alone forward and backward.  Returns everything the comparison needs."""
    from rot_mvgaze_amd import synth
    from rot_mvgaze_amd.arch import Variant
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    from rot_mvgaze_amd.model import MultiViewGaze
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    variant = Variant(**variant_kw) if variant_kw is not None else None
    raw = synth.make_state_dict(depth, 0, I, variant=variant) if variant is not None else synth.make_state_dict(depth, 0, I)
    sd = {k: np.array(v) for k, v in raw.items()}
    if fuser_scale != 1.0:
        for k in sd:
            if k.startswith("_img_fusers."):
                sd[k] = (sd[k] * np.float32(fuser_scale)).astype(np.float32)
    m = MultiViewGaze(depth, I, variant) if variant is not None else MultiViewGaze(depth, I)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m.to(dev()).train()
    m.ensure_layout()
    torch.manual_seed(seed)
    cf = m._fc_dim
    img_feat = (torch.rand(V, B, cf, device=dev()) * 2.0).contiguous()
    rot = rotation_matrix_2d(torch.rand(B * V, 2, device=dev()) - 0.5).reshape(B, V, 3, 3)
    head = m._head
    head.split, head.mixed = split, mixed
    lifted, feats, preds, tape = head.forward(img_feat, rot, True, True)
    gpred = torch.randn_like(preds)
    m._sink.active = False
    m._sink.begin()
    dimg = head.backward(tape, None, None, gpred, m._sink, None)
    m._sink.active = False
    torch.cuda.synchronize()
    return dict(m=m, sd=sd, variant=variant, img_feat=img_feat, rot=rot, feats=feats, preds=preds, tape=tape, gpred=gpred, dimg=dimg,
                V=V, B=B, I=I)


def _hidden_masks(tape, B, I):
    """(lifter, [fuser per iteration], [head per iteration]) hidden-layer ReLU patterns of the forward that wrote `tape`."""
    from rot_mvgaze_amd import ops
    V = tape["V"]
    hl_mask = (tape["hl"][0] > 0).cpu().view(V, B, -1)
    assert len(tape["saved"]) == I
    if tape["mode"] == "split":          # heads._forward_split: (xf, h, xh, hh, weight copies...) - h in (scaled) sp, hh fp32
        fuse_mask = [(ops.merge_sp(tape["saved"][it][1]) > 0).cpu().view(-1, B, tape["saved"][it][1].shape[-3] * 8) for it in range(I)]
        head_mask = [(tape["saved"][it][3] > 0).cpu().view(-1, B, tape["saved"][it][3].shape[-1]) for it in range(I)]
    else:                                # (input, [hidden], head input, [hidden], scales): fp32 hidden activations, one per hidden layer
        fuse_mask = [(tape["saved"][it][1][0] > 0).cpu().view(-1, B, tape["saved"][it][1][0].shape[-1]) for it in range(I)]
        head_mask = [(tape["saved"][it][3][0] > 0).cpu().view(-1, B, tape["saved"][it][3][0].shape[-1]) for it in range(I)]
    return hl_mask, fuse_mask, head_mask


def compare_with_oracle(run, tag, bars, storage=None):
    """The fp64 oracle with the forward's ReLU patterns against `run` (from run_head).
    bars: {"feat" / "pred" / "dimg" / "grad": (metric name, bar)}; every comparison is held to its group's bar, each group's
    smallest .. largest figure printed first.  ``storage`` = oracle.restatement.bf16_round: the oracle's Linears round their
    operands like the head's bf16 ("mixed") Linears.  Returns the printed lines."""
    from oracle import restatement as R
    m, sd, tape, V, B, I = run["m"], run["sd"], run["tape"], run["V"], run["B"], run["I"]
    feats, preds, gpred, dimg, variant = run["feats"], run["preds"], run["gpred"], run["dimg"], run["variant"]
    assert feats.shape[0] == I and preds.shape[0] == I and preds.shape[1:] == (V * (V - 1), B, 2)
    sd64 = {k: torch.from_numpy(v).double() for k, v in sd.items() if v.dtype == np.float32 and not k.startswith("_feat_extractor")}
    for t in sd64.values():                                 # (share_weights: one leaf per NAME; the sum over the names is compared)
        t.requires_grad_(True)
    f64 = [run["img_feat"][v].double().cpu().requires_grad_(True) for v in range(V)]
    r64 = run["rot"].double().cpu()
    hl_mask, fuse_mask, head_mask = _hidden_masks(tape, B, I)
    fig = Figures(tag)
    fn = {g: METRICS[bars[g][0]] for g in bars}
    R._LINEAR_Q = storage
    try:
        lift64 = [R.lift(sd64, f64[v], hl_mask[v]) for v in range(V)]
        total, p = 0.0, 0
        for (i, j) in R.view_pairs(V):
            masks = {}
            for it in range(I):
                masks[("fuse", it)] = [fuse_mask[it][2 * p], fuse_mask[it][2 * p + 1]]
                masks[("head", it)] = [head_mask[it][2 * p], head_mask[it][2 * p + 1]]
            o = R.fuse_pair(sd64, I, f64[i], f64[j], lift64[i], lift64[j], r64[:, i], r64[:, j], masks, variant)
            assert f"iter_{I}" not in o
            for it in range(I):
                for side in (0, 1):
                    d = 2 * p + side
                    fig.add("feat", fn["feat"](feats[it, d].cpu().reshape(B, -1), o[f"iter_{it}"][f"feat_{side}"].detach().reshape(B, -1)),
                            f"iteration {it} direction {d}")
                    fig.add("pred", fn["pred"](preds[it, d].cpu(), o[f"iter_{it}"][f"pred_gaze_{side}"].detach()), f"iteration {it} direction {d}")
                    total = total + (o[f"iter_{it}"][f"pred_gaze_{side}"] * gpred[it, d].double().cpu()).sum()
            p += 1
        total.backward()
    finally:
        R._LINEAR_Q = None
    for v in range(V):
        fig.add("dimg", fn["dimg"](dimg[v].cpu(), f64[v].grad), f"view {v}")
    groups = {}
    for k, prm in m.named_parameters(remove_duplicate=False):
        if not k.startswith("_feat_extractor"):
            groups.setdefault(id(prm), (prm, []))[1].append(k)
    seen_iters = set()
    for prm, names in groups.values():
        refs = [sd64[k].grad for k in names if sd64[k].grad is not None]
        if not refs:
            continue
        fig.add("grad", fn["grad"](m._grad_views[id(prm)].cpu(), sum(refs)), "+".join(names))
        seen_iters.update(int(k.split(".")[1]) for k in names if k.startswith(("_img_fusers.", "_gaze_estimators.")))
    assert seen_iters == set(range(I)), seen_iters            # every iteration's fuser and head has a gradient that was compared
    lines = [fig.report(g, bars[g][0], bars[g][1]) for g in ("feat", "pred", "dimg", "grad")]
    for g in ("feat", "pred", "dimg", "grad"):
        err, what = fig.worst(g)
        assert err < bars[g][1], (tag, g, what, err)
    return lines
