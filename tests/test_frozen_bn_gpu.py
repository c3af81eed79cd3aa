"""model.freeze_batchnorm: training steps that keep the backbone's BatchNorm on its running statistics (PyTorch's bn.eval() idiom
inside model.train()), on the fp32 model and on the bf16 path.

fp32      a train() + freeze_batchnorm step runs the launches of the eval() step with gradients: loss, every gradient and every
          buffer bit-identical to it, the grad-ready publish order the train-mode one.
bf16      against the CPU oracle with the same storage rounding (R.multiview_forward(..., training=False, masks, R.bf16_round),
          the HIP forward's ReLU pattern imposed) at tests/test_bf16_gpu.py's BF16_PRED_TOL / BF16_LOSS_TOL / BF16_GRAD_L2; every
          unit forward and every residual block backward teacher-forced on the CPU (the scheme of that file's
          _check_units_teacher_forced / _check_blocks_backward_teacher_forced with scale = gamma rsqrt(running_var + eps)) at
          OUT_RTOL / BWD_BLOCK_L2 - random-init ResNet-50 is held teacher-forced only, as that file explains; buffers, determinism,
          raw uint8 patches through a seeded TrainAugment, the fine-tuning boundary, Adam steps and host synchronisation.
Without the feature the attribute is inert: a train-mode step then moves the running statistics and the buffer tests fail.
Measured on an MI355X (profiles/r19_frozen_bn_errors.txt): ResNet-18 against the bf16-storage oracle predictions 6.0e-03, loss
1.7e-04, fusion-block gradients 8.8e-04 .. 2.6e-03 relative L2; teacher-forced backward worst 2.3e-02 (ResNet-18, 68
comparisons) and 3.5e-02 (ResNet-50, 175 comparisons), both the stem's weight gradient."""
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rot_mvgaze_amd import synth
from test_bf16_gpu import BF16_GRAD_L2, BF16_LOSS_TOL, BF16_PRED_TOL, BWD_BLOCK_L2, OUT_RTOL, _unit_input, close
from test_finetune_gpu import BB, freeze, in_prefix, is_bn_affine, launch_spy

pytestmark = pytest.mark.gpu

BN_EPS = 1e-5


def dev():
    return torch.device("cuda:0")


_SD = {}


def state(depth):
    if depth not in _SD:
        _SD[depth] = synth.make_state_dict(depth, 0, 3, perturb_bn=True)
    return _SD[depth]


def build(depth=18, train=True, frozen=True, bf16=True, **variant):
    from rot_mvgaze_amd.arch import Variant
    from rot_mvgaze_amd.model import FeatRotationSymm
    m = FeatRotationSymm(backbone_depth=depth, num_iter=3, **variant)
    sd = synth.make_state_dict(depth, 0, 3, perturb_bn=True, variant=Variant(**variant)) if variant else state(depth)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    m.to(dev())
    if bf16:
        m.compute_dtype = torch.bfloat16
    m.freeze_batchnorm = frozen
    return m.train() if train else m.eval()


def inputs(batch, hw, seed=1234):
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    inp = synth.make_inputs(batch, 2, seed, hw)
    img, hp, gt = (torch.from_numpy(inp[k]).to(dev()) for k in ("img", "head_pose", "gt_gaze"))
    return {"img_0": img[:, 0].contiguous(), "img_1": img[:, 1].contiguous(),
            "rot_0": rotation_matrix_2d(hp[:, 0].contiguous()), "rot_1": rotation_matrix_2d(hp[:, 1].contiguous()),
            "gt_gaze": gt[:, 0].contiguous(), "gt_gaze_1": gt[:, 1].contiguous()}


def metrics():
    from rot_mvgaze_amd.losses import IterationLoss, StereoL1Loss
    return IterationLoss(StereoL1Loss(rel_weight=0.01, reference_decay=1.0, distance_metric="angular_error",
                                      pred_gaze_key="pred_gaze"), iter_decay=0.5)


def buffers(m):
    return {k: v.detach().clone() for k, v in m.named_buffers()}


def assert_buffers_equal(before, m):
    after = dict(m.named_buffers())
    assert set(before) == set(after)
    for k, v in before.items():
        assert torch.equal(v, after[k]), f"buffer {k} changed"


def step(m, data):
    """forward + loss + backward from empty gradients; returns (loss, gradients by name)."""
    for p in m.parameters():
        p.grad = None
    loss = metrics()(m(dict(data)))
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


# ---------------------------------------------------------------- fp32
def test_fp32_frozen_step_is_the_eval_step_bit_for_bit():
    """ResNet-18, default variant, B = 4, 64 px."""
    data = inputs(4, 64)
    ev = build(train=False, frozen=False, bf16=False)
    before = buffers(ev)
    loss_e, grads_e = step(ev, data)
    fr = build(train=True, frozen=True, bf16=False)
    assert fr.training and fr.freeze_batchnorm
    loss_f, grads_f = step(fr, data)
    call = fr._backbone._last_call
    assert call.training is False and call.train_step is True and call.taped and not call.sp and not call.stem_rw
    assert torch.equal(loss_e, loss_f)
    assert set(grads_e) == set(grads_f) and len(grads_f) > 60
    for k, g in grads_e.items():
        assert torch.equal(g, grads_f[k]), k
    assert_buffers_equal(before, ev)
    assert_buffers_equal(before, fr)
    assert any(k.endswith("num_batches_tracked") for k in before)


def test_fp32_frozen_step_publishes_gradients_in_train_mode_order():
    m = build(train=True, frozen=False, bf16=False)
    names = {id(p): k for k, p in m.named_parameters()}
    data = inputs(2, 64)

    def batches(frozen):
        m.freeze_batchnorm = frozen
        seen = []
        m._on_grads_ready = lambda ps: seen.append([names[id(p)] for p in ps])
        m.zero_grad(set_to_none=True)
        metrics()(m(dict(data))).backward()
        torch.cuda.synchronize()
        m._on_grads_ready = None
        return seen
    fr, tr = batches(True), batches(False)
    assert len(fr) > 5 and fr == tr


def test_flag_has_no_effect_in_eval_and_bf16_eval_backward_is_still_refused():
    data = inputs(2, 64)
    a, b = build(train=False, frozen=True, bf16=False), build(train=False, frozen=False, bf16=False)
    la, ga = step(a, data)
    lb, gb = step(b, data)
    assert torch.equal(la, lb) and all(torch.equal(g, gb[k]) for k, g in ga.items())
    m = build(train=False, frozen=True, bf16=True)
    loss = metrics()(m(dict(data)))
    with pytest.raises(NotImplementedError, match="bf16"):
        loss.backward()


# ---------------------------------------------------------------- bf16: the oracle
def captured_masks(m, V):
    """ReLU patterns of the HIP forward of a bf16 tape, in the order the oracle applies its ReLUs: residual units carry bits - 8
    elements per byte on this path, the layout mvg_bn_apply_bits_bf16 writes - the others their stored activation, the stem
    fma(y, scale, shift) > 0."""
    bt, ht = m._last_backbone_tape, m._last_head_tape
    relu_units = [u for u in bt["units"] if u.relu]

    def unit_mask(u, v):
        if u.relu_bits is not None:
            assert u.relu_bits.numel() * 8 == u.y.numel()
            bits = u.relu_bits.view(u.y.shape[0], -1)[v]
            on = ((bits[:, None] >> torch.arange(8, device=bits.device, dtype=torch.uint8)[None, :]) & 1).bool()
            return on.reshape(u.y.shape[1:])
        if u.out is not None:
            return u.out[v].contiguous() > 0
        scale, shift = u.pool[1], u.pool[2]
        return (u.y[v].double() * scale[v].double() + shift[v].double()) > 0
    masks = {"backbone": [iter([unit_mask(u, v).permute(0, 3, 1, 2).cpu() for u in relu_units]) for v in range(V)]}
    B = bt["B"]
    hl = (ht["hl"][0] > 0).cpu()
    masks["lift"] = [hl[v * B:(v + 1) * B] for v in range(V)]
    D = V * (V - 1)
    for it, (X, H1, Xh, Hh, _scales) in enumerate(ht["saved"]):
        h1, hh = (H1[0] > 0).cpu(), (Hh[0] > 0).cpu()
        masks[("fuse", it)] = [h1[d * B:(d + 1) * B] for d in range(D)]
        masks[("head", it)] = [hh[d * B:(d + 1) * B] for d in range(D)]
    return masks


def multiview_step(depth, V, B, hw):
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    from rot_mvgaze_amd.losses import MultiViewIterationLoss
    from rot_mvgaze_amd.model import MultiViewGaze
    m = MultiViewGaze(depth, 3)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state(depth).items()})
    m.to(dev()).train()
    m.compute_dtype = torch.bfloat16
    m.freeze_batchnorm = True
    m._debug_keep_tapes = True
    inp = synth.make_inputs(B, V, 5, hw)
    img, hp, gt = (torch.from_numpy(inp[k]) for k in ("img", "head_pose", "gt_gaze"))
    rot_d = rotation_matrix_2d(hp.reshape(-1, 2).to(dev())).reshape(B, V, 3, 3)
    out = m.forward_multiview([img[:, v].contiguous().to(dev()) for v in range(V)], rot_d)
    crit = MultiViewIterationLoss(rel_weight=0.01, reference_decay=1.0, iter_decay=0.5)
    return m, out, crit, img, hp, gt


def test_bf16_frozen_step_against_the_bf16_storage_oracle():
    """ResNet-18, V = 2, B = 8, 96 px."""
    from oracle import restatement as R
    depth, V, B, hw = 18, 2, 8, 96
    m, out, crit, img, hp, gt = multiview_step(depth, V, B, hw)
    before = {k: torch.from_numpy(np.array(v)) for k, v in state(depth).items() if "running" in k or "tracked" in k}
    masks = captured_masks(m, V)
    loss = crit(out, gt.to(dev()))
    loss.backward()
    sd = {k: torch.from_numpy(np.array(v)) for k, v in state(depth).items()}
    leaves = {k: v.requires_grad_(True) for k, v in sd.items() if v.dtype == torch.float32 and "running" not in k}
    rot = R.rotation_matrix_2d(hp.reshape(-1, 2)).reshape(B, V, 3, 3)
    oo = R.multiview_forward(sd, img, rot, depth, 3, False, masks, R.bf16_round)
    ol = R.multiview_loss(oo, gt, iter_decay=0.5, rel_weight=0.01, reference_decay=1.0)
    ol.backward()
    worst = 0.0
    for pr in R.view_pairs(V):
        for it in range(3):
            for k in ("pred_gaze_0", "pred_gaze_1"):
                got, ref = out["pairs"][pr][f"iter_{it}"][k].detach().cpu().double(), oo["pairs"][pr][f"iter_{it}"][k].detach().double()
                worst = max(worst, float((got - ref).abs().max() / (ref.abs().max() + 1e-30)))
    le = abs(loss.item() - ol.item()) / abs(ol.item())
    print(f"FROZEN-BN bf16 r18 vs the bf16-storage oracle: pred {worst:.3e} (bar {BF16_PRED_TOL}), loss {le:.3e} (bar {BF16_LOSS_TOL})")
    assert worst <= BF16_PRED_TOL and le <= BF16_LOSS_TOL
    params = dict(m.named_parameters())
    for k in ("_lifter._lifter.blocks.0.0.weight", "_img_fusers.0._fuser.blocks.0.0.weight", "_gaze_estimators.1.blocks.1.0.weight"):
        got, ref = params[k].grad.detach().cpu().double(), leaves[k].grad.double()
        err = float((got - ref).norm() / (ref.norm() + 1e-30))
        print(f"FROZEN-BN bf16 r18 grad {k}: relative L2 {err:.3e} (bar {BF16_GRAD_L2})")
        assert err <= BF16_GRAD_L2, f"grad {k}: relative L2 {err:.3e}"
    for k, v in before.items():                                       # the oracle in eval mode moved none either
        assert torch.equal(m.state_dict()[k].cpu(), v) and torch.equal(sd[k], v), k


# ---------------------------------------------------------------- bf16: teacher-forced
def check_units_teacher_forced(m, img_feat):
    """test_bf16_gpu._check_units_teacher_forced for units on the running statistics: every conv output (the bf16 rounding of the
    fp32 result of the unit's own recorded input), activation = round(relu(y scale + shift [+ identity])) with scale = gamma /
    sqrt(running_var + eps), shift = beta - running_mean scale, the fused stem tail and the average pool."""
    tape = m._last_backbone_tape
    units = tape["units"]
    P = dict(m.named_parameters())
    Bf = dict(m.named_buffers())
    q = lambda t: t.to(torch.bfloat16).float()
    identity_of, affine_of = {}, {}
    for idx, ds_idx in tape["blocks"]:
        identity_of[idx[-1]] = ("ds", ds_idx) if ds_idx is not None else ("x", idx[0])
    for ui, u in enumerate(units):
        c, d = u.spec, u.desc
        assert not u.trained and not u.stem_rw
        G, N = u.y.shape[0], u.y.shape[1]
        x = _unit_input(u).reshape(G * N, d.h, d.w, -1).permute(0, 3, 1, 2)[:, :c.cin]
        w = q(P[c.name + ".weight"].detach().float().cpu().contiguous())
        y_ref = F.conv2d(x, w, None, c.stride, c.pad)
        y_got = u.y.float().cpu().reshape(G * N, d.ho, d.wo, c.cout).permute(0, 3, 1, 2)
        close(y_got, y_ref, OUT_RTOL, f"{c.name}: conv output")
        scale = P[c.bn + ".weight"].detach().cpu() / torch.sqrt(Bf[c.bn + ".running_var"].cpu() + BN_EPS)
        shift = P[c.bn + ".bias"].detach().cpu() - Bf[c.bn + ".running_mean"].cpu() * scale
        sc, sh = scale.reshape(1, c.cout, 1, 1), shift.reshape(1, c.cout, 1, 1)
        act = y_got * sc + sh
        affine_of[ui] = (y_got, sc, sh)
        if ui in identity_of:
            kind, j = identity_of[ui]
            if kind == "ds":
                yd, scd, shd = affine_of[j]
                act = act + (yd * scd + shd)
            else:
                act = act + units[j].x_in.float().cpu().reshape(G * N, d.ho, d.wo, c.cout).permute(0, 3, 1, 2)
        if u.relu:
            act = F.relu(act)
        if u.out is not None:
            got = u.out.float().cpu().reshape(G * N, d.ho, d.wo, c.cout).permute(0, 3, 1, 2)
            close(got, q(act), OUT_RTOL, f"{c.name}: activation")
        elif ui == 0:
            nxt = units[1].x_in.float().cpu()
            got = nxt.reshape(G * N, nxt.shape[2], nxt.shape[3], c.cout).permute(0, 3, 1, 2)
            close(got, q(F.max_pool2d(act, 3, 2, 1)), OUT_RTOL, "stem: pooled activation")
    last = units[tape["blocks"][-1][0][-1]]
    G, N = last.out.shape[0], last.out.shape[1]
    close(img_feat.detach().cpu(), last.out.float().cpu().reshape(G, N, -1, last.out.shape[-1]).mean(2), 1e-5, "average pool")
    assert len(units) == sum(1 for _ in m._backbone.spec.all_convs())


def check_blocks_backward_teacher_forced(m, tape, dfeat):
    """test_bf16_gpu._check_blocks_backward_teacher_forced with BatchNorm on the running statistics: every residual block's
    recorded bf16 input through the block on the CPU (fp64 autograd, the same storage rounding), the recorded gradient of its
    output back-propagated; the result must reproduce the recorded gradient of its input - NOT masked by the unit it feeds: a
    frozen step's backward-data launches carry no fused reduce, the one-pass BatchNorm backward applies that mask - and the block's
    weight / BatchNorm gradients, at BWD_BLOCK_L2 relative L2."""
    units, blocks, dbg = tape["units"], tape["blocks"], tape["debug"]
    P = dict(m.named_parameters())
    Bf = dict(m.named_buffers())
    spec = m._backbone.spec
    q = lambda t: t.to(torch.bfloat16).to(t.dtype)
    G, N = units[0].x_in.shape[0], units[0].x_in.shape[1]
    Hc, Wc = tape["final_hw"]
    g_out = q((dfeat.detach().cpu().double() / (Hc * Wc))[:, :, None, None, :].expand(G, N, Hc, Wc, dfeat.shape[-1]))
    assert len(dbg) == len(blocks)
    nchw = lambda t: t.double().permute(0, 3, 1, 2)

    def unit(x, c, wts, relu, identity=None, stored=True):
        w = wts.setdefault(c.name + ".weight", q(P[c.name + ".weight"].detach().cpu().double().contiguous()).requires_grad_(True))
        ga = wts.setdefault(c.bn + ".weight", P[c.bn + ".weight"].detach().cpu().double().requires_grad_(True))
        be = wts.setdefault(c.bn + ".bias", P[c.bn + ".bias"].detach().cpu().double().requires_grad_(True))
        y = F.conv2d(x, w, None, c.stride, c.pad)
        scale = ga * torch.rsqrt(Bf[c.bn + ".running_var"].cpu().double() + BN_EPS)
        o = q(y) * scale[None, :, None, None] + (be - Bf[c.bn + ".running_mean"].cpu().double() * scale)[None, :, None, None]
        if identity is not None:
            o = o + identity
        if not stored:
            return o
        return q(F.relu(o)) if relu else q(o)

    report = []

    def compare(wts, what):
        for name, leaf in wts.items():
            got = P[name].grad.detach().cpu().double()
            report.append((float((got - leaf.grad).norm() / (leaf.grad.norm() + 1e-30)), f"{what}: gradient of {name}"))

    for bi in range(len(blocks) - 1, -1, -1):
        idx, ds_idx = blocks[bi]
        blk = spec.blocks[bi]
        g_in_rec = dbg[len(blocks) - 1 - bi].float().cpu()
        x_rec = units[idx[0]].x_in.float().cpu()
        wts, dxs = {}, []
        for g in range(G):
            x = nchw(x_rec[g]).requires_grad_(True)
            o = x
            for c in blk.convs[:-1]:
                o = unit(o, c, wts, True)
            identity = unit(x, blk.downsample, wts, False, None, False) if blk.downsample is not None else x
            o = unit(o, blk.convs[-1], wts, True, identity)
            o.backward(nchw(g_out[g]))
            dxs.append(x.grad.permute(0, 2, 3, 1))
        dx = torch.stack(dxs)
        report.append((float((g_in_rec.double() - dx).norm() / (dx.norm() + 1e-30)), f"block {bi}: gradient wrt the block input"))
        compare(wts, f"block {bi}")
        g_out = g_in_rec.double()
    c, wts = spec.stem, {}
    x_rec = _unit_input(units[0])[..., :3]
    for g in range(G):
        o = F.max_pool2d(unit(nchw(x_rec[g]), c, wts, True), 3, 2, 1)
        o.backward(nchw(g_out[g]))
    compare(wts, "stem")
    worst = max(report)
    print(f"FROZEN-BN teacher-forced backward, {len(report)} comparisons: worst {worst[0]:.3e} ({worst[1]}), bar {BWD_BLOCK_L2}")
    bad = [(e, w) for e, w in report if e > BWD_BLOCK_L2]
    assert not bad, "teacher-forced backward: " + "; ".join(f"{w} {e:.2e}" for e, w in sorted(bad, reverse=True)[:6])


@pytest.mark.parametrize("depth", [18, 50], ids=["r18", "r50"])
def test_bf16_frozen_step_teacher_forced(depth):
    """V = 2, B = 4, 96 px: every unit forward and every residual block backward from its own recorded input."""
    m, out, crit, img, hp, gt = multiview_step(depth, 2, 4, 96)
    check_units_teacher_forced(m, out["img_feat"])                       # before backward: it releases the activations
    tape = m._last_backbone_tape
    assert tape["call"].train_step and not tape["call"].training and not tape["call"].stem_rw
    tape["debug"] = []
    out["img_feat"].retain_grad()
    crit(out, gt.to(dev())).backward()
    check_blocks_backward_teacher_forced(m, tape, out["img_feat"].grad)


# ---------------------------------------------------------------- bf16: buffers, determinism
def _frozen_adam_step(m):
    from rot_mvgaze_amd.optim import Adam
    opt = Adam(m.parameters(), lr=1e-4)
    loss, grads = step(m, inputs(4, 64))
    start = m.param_arena().clone()
    opt.step()
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and len(grads) > 60
    assert not torch.equal(m.param_arena(), start)


def test_bf16_frozen_step_leaves_every_buffer_untouched():
    """Every buffer of the model - running statistics and num_batches_tracked of all 20 BatchNorm layers - bit-identical after
    forward + backward + Adam."""
    m = build()
    before = buffers(m)
    assert sum(k.endswith("num_batches_tracked") for k in before) == sum(k.endswith("running_var") for k in before) == 20
    _frozen_adam_step(m)
    assert_buffers_equal(before, m)


def test_bf16_frozen_step_share_feature_only_the_backbone_is_frozen():
    """The share_feature variant: the backbone's BatchNorm buffers stay bit-identical; IntensityBatchNorm is not an
    nn.BatchNorm2d, the idiom (bn.eval() on the BatchNorm2d modules) would not reach it, and the head receives model.training
    unchanged - its running_mean follows the training step, as MultiViewGaze.freeze_batchnorm documents.  In eval() with the
    flag set nothing moves."""
    m = build(share_feature=True)
    before = buffers(m)
    ibn = [k for k in before if "_batchnorm.running_mean" in k]
    assert len(ibn) == 3 and len(before) > 60
    _frozen_adam_step(m)
    after = dict(m.named_buffers())
    for k, v in before.items():
        if k in ibn:
            assert not torch.equal(v, after[k]), f"{k}: the head did not run in train mode"
        else:
            assert torch.equal(v, after[k]), f"buffer {k} changed"
    m.eval()
    now = buffers(m)
    with torch.no_grad():
        metrics()(m(dict(inputs(4, 64))))
    assert_buffers_equal(now, m)


def test_bf16_flag_off_the_next_step_updates_the_statistics():
    m = build()
    before = buffers(m)
    data = inputs(4, 64)
    step(m, data)
    assert_buffers_equal(before, m)
    m.freeze_batchnorm = False
    step(m, data)
    after = dict(m.named_buffers())
    assert int(after[BB + "bn1.num_batches_tracked"]) == 2                 # V = 2: one per view call
    assert all(int(v) == 2 for k, v in after.items() if k.endswith("num_batches_tracked"))
    moved = sum(int(not torch.equal(v, before[k])) for k, v in after.items() if k.endswith("running_mean") and k.startswith(BB))
    assert moved == 20                                                     # ResNet-18: every BatchNorm layer


def test_bf16_frozen_backward_run_to_run_determinism():
    m = build()
    data = inputs(8, 96, seed=5)
    (l0, g0), (l1, g1) = step(m, data), step(m, data)
    assert torch.equal(l0, l1) and len(g0) > 60
    for k, g in g0.items():
        assert torch.equal(g, g1[k]), k


# ---------------------------------------------------------------- bf16: raw uint8 patches
def test_bf16_frozen_step_from_raw_patches_with_a_seeded_augment():
    """The frozen step on BGR uint8 patches with model.input_augment (erase on) equals the step fed TrainAugment.apply(out="nchw")
    with the same draws as fp32 input - loss and every gradient, bit for bit; without an augment it is refused as ever."""
    from rot_mvgaze_amd.augment import RandomMultiErasing, TrainAugment
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    B, hw = 2, 64
    rng = np.random.RandomState(9)
    u8 = [torch.from_numpy(rng.randint(0, 256, (B, hw, hw, 3)).astype(np.uint8)).to(dev()) for _ in range(2)]
    inp = synth.make_inputs(B, 2, 1234, hw)
    hp, gt = (torch.from_numpy(inp[k]).to(dev()) for k in ("head_pose", "gt_gaze"))
    rest = {"rot_0": rotation_matrix_2d(hp[:, 0].contiguous()), "rot_1": rotation_matrix_2d(hp[:, 1].contiguous()),
            "gt_gaze": gt[:, 0].contiguous(), "gt_gaze_1": gt[:, 1].contiguous()}
    aug = TrainAugment(erase=RandomMultiErasing([0.3, 0.6], 0.5, [0.1, 0.34]))

    def seed():
        torch.manual_seed(77), random.seed(77), np.random.seed(77)
    a = build()
    a.input_size, a.input_augment, a.input_bgr = None, aug, True
    before = buffers(a)
    seed()
    la, ga = step(a, dict(rest, img_0=u8[0], img_1=u8[1]))
    assert not a._backbone._stem_rw                       # no statistics, no row-window stem: the augment wrote the NHWC8 operand
    seed()
    f32 = [aug.apply(u, aug.draw(B, hw, hw), out="nchw", bgr=True) for u in u8]
    b = build()
    lb, gb = step(b, dict(rest, img_0=f32[0], img_1=f32[1]))
    assert torch.equal(la, lb) and torch.isfinite(la)
    assert set(ga) == set(gb) and len(ga) > 60
    for k, g in ga.items():
        assert torch.equal(g, gb[k]), k
    assert ga[BB + "conv1.weight"].abs().max() > 0
    # the augment did something: the un-augmented patches give another loss
    c = build()
    c.input_size, c.input_bgr = None, True
    c.eval()
    with torch.no_grad():
        plain = metrics()(c(dict(rest, img_0=u8[0], img_1=u8[1])))
    assert not torch.equal(plain, la)
    assert_buffers_equal(before, a)
    a.input_augment = None
    with pytest.raises(NotImplementedError, match="inference only"):
        a(dict(rest, img_0=u8[0], img_1=u8[1]))


# ---------------------------------------------------------------- bf16: the fine-tuning boundary
def test_bf16_frozen_step_below_the_boundary_is_silent_and_no_fused_reduce_anywhere(monkeypatch):
    from rot_mvgaze_amd import ops
    fused = []
    real = ops.conv_dgrad_bf16_bnreduce
    monkeypatch.setattr(ops, "conv_dgrad_bf16_bnreduce", lambda *a, **k: (fused.append(1), real(*a, **k))[1])
    data = inputs(4, 64)
    # nothing frozen: a train-mode step uses the fused launch (the spy sees it), a frozen-BatchNorm step never does
    step(build(frozen=False), data)
    assert fused
    del fused[:]
    m = build()
    with launch_spy() as calls:
        _, ref = step(m, data)
    assert not fused and ("_stem_bn_bwd", BB + "conv1") in calls and [c for c in calls if in_prefix(c[1])]
    # everything below layer3 frozen
    m = build()
    frozen = freeze(m, in_prefix)
    with launch_spy() as calls:
        _, grads = step(m, data)
    assert not fused and calls
    assert [c for c in calls if in_prefix(c[1])] == []
    assert [c for c in calls if c[0] == "_dgrad" and c[1] in (BB + "layer3.0.conv1", BB + "layer3.0.downsample.0")] == []
    assert ("_wgrad", BB + "layer3.0.conv1") in calls and ("_wgrad", BB + "layer3.0.downsample.0") in calls
    assert set(grads) == set(ref) - frozen
    for k, g in grads.items():                              # running statistics do not depend on what is frozen: the same bits
        assert torch.equal(g, ref[k]), k
    # only the BatchNorm affine parameters frozen: the conv weights still get gradients, no BatchNorm gradient appears
    m = build()
    frozen = freeze(m, is_bn_affine)
    assert len(frozen) == 2 * 20
    with launch_spy() as calls:
        _, grads = step(m, data)
    assert not fused
    assert len([c for c in calls if c[0] == "_wgrad"]) == 20 and not any(k in grads for k in frozen)
    convs = [k for k in ref if k.startswith(BB) and k not in frozen]
    assert len(convs) == 20
    for k in convs:
        assert torch.equal(grads[k], ref[k]), k


# ---------------------------------------------------------------- bf16: optimisation, host behaviour
def test_bf16_frozen_fine_tuning_lowers_the_loss():
    from rot_mvgaze_amd.optim import Adam
    m = build()
    before = buffers(m)
    opt = Adam(m.parameters(), lr=1e-4)
    d = inputs(4, 64, seed=3)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = metrics()(m(dict(d)))
        loss.backward()
        opt.step()
        losses.append(loss.item())
    with torch.no_grad():
        losses.append(metrics()(m(dict(d))).item())
    assert losses[-1] < losses[0], losses
    assert_buffers_equal(before, m)


def test_bf16_frozen_step_does_not_synchronise_the_host():
    from rot_mvgaze_amd.optim import Adam
    m = build()
    crit = metrics()
    opt = Adam(m.parameters(), lr=1e-4, weight_decay=1e-6)
    d = inputs(4, 64)

    def one():
        opt.zero_grad()
        crit(m(dict(d))).backward()
        opt.step()
    one()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        one()
        one()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
