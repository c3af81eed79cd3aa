"""Backward in eval mode (model.eval() with gradients on): BatchNorm differentiated through its RUNNING statistics, as
autograd does for F.batch_norm(training=False) in the reference.  The one-pass kernels (mvg_bn_eval_bwd,
mvg_bn_relu_maxpool_eval_bwd) against fp64 numpy; whole-model gradients against the fp64 oracle in eval mode with the
HIP forward's ReLU pattern imposed; buffers untouched, determinism, grad-ready order, no host synchronisation, a short
fine-tuning run; the bf16 path still refuses."""
import os
from collections import defaultdict

import numpy as np
import pytest
import torch

import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd import ops, synth

pytestmark = pytest.mark.gpu
TOL = 1e-4       # loss and predictions
GTOL = 2e-4      # parameter and image gradients, max-norm relative, same ReLU pattern on both sides
KTOL = 1e-6      # the kernels against fp64 numpy
EPS = 1e-5

VARIANTS = {
    "share_weights": dict(share_weights=True),
    "ignore_rotmat": dict(ignore_rotmat=True),
    "encode_rotmat": dict(encode_rotmat=True),
    "share_feature": dict(share_feature=True),
    "share_weights_encode_rotmat": dict(share_weights=True, encode_rotmat=True),
}


def dev():
    return torch.device("cuda:0")


def build(depth, seed=0, train=False, **variant):
    from rot_mvgaze_amd.arch import Variant
    from rot_mvgaze_amd.model import FeatRotationSymm
    m = FeatRotationSymm(backbone_depth=depth, num_iter=3, **variant)
    kw = dict(variant=Variant(**variant)) if variant else {}
    sd = synth.make_state_dict(depth, seed, 3, perturb_bn=True, **kw)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    m.to(dev())
    return (m.train() if train else m.eval()), sd


def inputs(batch, hw, seed=1234, views=2):
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    inp = synth.make_inputs(batch, views, seed, hw)
    img, hp, gt = (torch.from_numpy(inp[k]).to(dev()) for k in ("img", "head_pose", "gt_gaze"))
    return {"img_0": img[:, 0].contiguous(), "img_1": img[:, 1].contiguous(),
            "rot_0": rotation_matrix_2d(hp[:, 0].contiguous()), "rot_1": rotation_matrix_2d(hp[:, 1].contiguous()),
            "gt_gaze": gt[:, 0].contiguous(), "gt_gaze_1": gt[:, 1].contiguous()}


def metrics():
    from rot_mvgaze_amd.losses import IterationLoss, StereoL1Loss
    return IterationLoss(StereoL1Loss(rel_weight=0.01, reference_decay=1.0, distance_metric="angular_error",
                                      pred_gaze_key="pred_gaze"), iter_decay=0.5)


def rel_err(got, ref):
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    ref = ref.detach().cpu().double().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30))


def rel_close(got, ref, tol, what):
    e = rel_err(got, ref)
    assert e <= tol, f"{what}: max-norm relative error {e:.3e} > {tol}"


def _captured_masks(m, V=2, head=True):
    """ReLU patterns of the HIP forward, in the order the oracle applies its ReLUs (test_model_gpu.py's helper for the
    fp32 eval tape: residual units carry bits, the others their stored activation, the stem fma(y, scale, shift))."""
    bt, ht = m._last_backbone_tape, m._last_head_tape
    relu_units = [u for u in bt["units"] if u.relu]

    def unit_mask(u, v):
        if getattr(u, "relu_bits", None) is not None:
            G = u.y.shape[0]
            bits = u.relu_bits.view(G, -1)[v]
            on = ((bits[:, None] >> torch.arange(4, device=bits.device, dtype=torch.uint8)[None, :]) & 1).bool()
            return on.reshape(u.y.shape[1:])
        if u.out is not None:
            return u.out[v].contiguous() > 0
        scale, shift = u.pool[1], u.pool[2]
        return (u.y[v].double() * scale[v].double() + shift[v].double()) > 0
    masks = {"backbone": [iter([unit_mask(u, v).permute(0, 3, 1, 2).cpu() for u in relu_units]) for v in range(V)]}
    B = bt["B"]

    def f32(t):
        return ops.merge_sp(t) if t.dtype == torch.float16 else t
    hl = (f32(ht["hl"][0]) > 0).cpu()
    masks["lift"] = [hl[v * B:(v + 1) * B] for v in range(V)]
    if not head:
        return masks
    D = V * (V - 1)
    for it, rec in enumerate(ht["saved"]):
        if ht.get("mode") == "split":
            H1, Hh = [rec[1]], [rec[3]]
        else:
            (X, H1, Xh, Hh, _scales) = rec
        h1, hh = (f32(H1[0]) > 0).cpu(), (f32(Hh[0]) > 0).cpu()
        masks[("fuse", it)] = [h1[d * B:(d + 1) * B] for d in range(D)]
        masks[("head", it)] = [hh[d * B:(d + 1) * B] for d in range(D)]
    return masks


def _oracle_leaves(sd):
    sd = {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}
    sd = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in sd.items()}
    leaves = {k: v.requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and "running" not in k}
    return sd, leaves


def _grad_errors(m, leaves):
    """(max-norm relative error, name) per parameter; shared parameters against the sum over their names."""
    names = defaultdict(list)
    params = {}
    for k, p in m.named_parameters(remove_duplicate=False):
        names[id(p)].append(k)
        params[id(p)] = p
    errs = []
    for pid, ks in names.items():
        refs = [leaves[k].grad for k in ks if leaves[k].grad is not None]
        p = params[pid]
        if not refs:
            assert p.grad is None, ks
            continue
        errs.append((rel_err(p.grad, sum(refs)), ks[0]))
    return sorted(errs, reverse=True)


def _buffers(m):
    return {k: v.detach().clone() for k, v in m.named_buffers()}


def _assert_buffers_equal(before, m):
    after = dict(m.named_buffers())
    assert set(before) == set(after)
    for k, v in before.items():
        assert torch.equal(v, after[k]), f"buffer {k} changed"


# ------------------------------------------------------------------------------------------ kernels vs fp64 numpy
def _rand(rng, *shape, loc=0.0, scale=1.0):
    return (rng.standard_normal(shape) * scale + loc).astype(np.float32)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _bn_params(rng, c):
    gamma = _rand(rng, c, loc=1.0, scale=0.3)
    rm = _rand(rng, c, scale=0.5)
    rv = (rng.random(c) * 2.0 + 0.05).astype(np.float32)
    return gamma, rm, rv


def _eval_ref(dz, y, gamma, rm, rv):
    """dz [..., c] (masked), y [..., c]: dy, dgamma, dbeta in fp64."""
    dz, y = dz.astype(np.float64), y.astype(np.float64)
    inv = 1.0 / np.sqrt(rv.astype(np.float64) + EPS)
    dy = dz * (gamma.astype(np.float64) * inv)
    flat = dz.reshape(-1, dz.shape[-1])
    xhat = ((y - rm.astype(np.float64)) * inv).reshape(-1, dz.shape[-1])
    return dy, (flat * xhat).sum(0), flat.sum(0)


KCASES = [(1, 37, 64, "none"), (2, 1001, 256, "act"), (3, 777, 128, "bits"), (8, 129, 64, "affine"),
          (5, 3137, 2048, "bits"), (4, 513, 512, "affine"), (2, 49, 1024, "act"), (7, 95, 64, "bits")]


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("alias", ["separate", "dy_is_g", "dy_is_g_with_dz", "dz_is_g"])
@pytest.mark.parametrize("groups,rows,c,mask", KCASES, ids=[f"G{g}_r{r}_c{c}_{m}" for g, r, c, m in KCASES])
def test_bn_eval_bwd_kernel_against_numpy(groups, rows, c, mask, alias, accumulate):
    rng = np.random.default_rng(groups * 1000 + rows + c)
    g = _rand(rng, groups, rows, c, loc=0.3)
    y = _rand(rng, groups, rows, c, loc=0.2, scale=1.5)
    gamma, rm, rv = _bn_params(rng, c)
    kw = {}
    if mask == "none":
        on = np.ones_like(g, dtype=bool)
    elif mask == "act":
        act = _rand(rng, groups, rows, c)
        on = act > 0
        kw["act"] = _t(act)
    elif mask == "affine":
        sc, sh = _rand(rng, groups, c), _rand(rng, groups, c, scale=0.5)
        on = (y.astype(np.float64) * sc[:, None, :].astype(np.float64) + sh[:, None, :].astype(np.float64)) > 0
        kw["relu_affine"] = (_t(sc), _t(sh))
    else:              # the bytes bn_apply_bits records for a residual unit
        y2, res = _t(_rand(rng, groups, rows, c)), _t(_rand(rng, groups, rows, c))
        sc, sh = _t(_rand(rng, groups, c)), _t(_rand(rng, groups, c, scale=0.5))
        out = torch.empty_like(y2)
        kw["relu_bits"] = ops.bn_apply_bits(y2, sc, sh, res, out, groups, rows, c)
        on = (out > 0).cpu().numpy()
    dy_ref, dg_ref, db_ref = _eval_ref(g * on, y, gamma, rm, rv)
    g_d, y_d = _t(g), _t(y)
    dz_d = None
    if alias == "separate":
        dy_d = torch.empty_like(g_d)
        dz_d = torch.empty_like(g_d)
    elif alias == "dy_is_g":
        dy_d = g_d
    elif alias == "dy_is_g_with_dz":
        dy_d = g_d
        dz_d = torch.empty_like(g_d)
    else:
        dy_d = torch.empty_like(g_d)
        dz_d = g_d
    dg0, db0 = _rand(rng, c), _rand(rng, c)
    dgamma, dbeta = _t(dg0), _t(db0)
    ops.bn_eval_bwd(g_d, y_d, _t(gamma), _t(rm), _t(rv), EPS, groups, rows, c, dy_d, dgamma, dbeta, accumulate,
                    dz_out=dz_d, **kw)
    torch.cuda.synchronize()
    rel_close(dy_d, dy_ref, KTOL, "dy")
    if dz_d is not None:
        assert torch.equal(dz_d.cpu(), torch.from_numpy(g * on)), "dz_out is not the masked gradient"
    base_g, base_b = (dg0.astype(np.float64), db0.astype(np.float64)) if accumulate else (0.0, 0.0)
    rel_close(dgamma, base_g + dg_ref, KTOL, "dgamma")
    rel_close(dbeta, base_b + db_ref, KTOL, "dbeta")


PCASES = [(2, 3, 13, 11, 64), (1, 2, 16, 16, 64), (3, 1, 7, 9, 32), (2, 2, 112, 112, 64)]


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("groups,n,h,w,c", PCASES, ids=[f"G{g}_n{n}_{h}x{w}_c{c}" for g, n, h, w, c in PCASES])
def test_bn_relu_maxpool_eval_bwd_kernel_against_numpy(groups, n, h, w, c, accumulate):
    """The stem tail: odd and even maps (edge windows that hang over the border), groups 1-3."""
    rng = np.random.default_rng(h * 100 + w + c)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    y = _rand(rng, groups, n, h, w, c, loc=0.1)
    gamma, rm, rv = _bn_params(rng, c)
    beta = _rand(rng, c, scale=0.3)
    y_d = _t(y)
    scale, shift = torch.empty(groups, c, device=dev()), torch.empty(groups, c, device=dev())
    ops.bn_eval_affine(groups, c, _t(gamma), _t(beta), _t(rm), _t(rv), EPS, scale, shift)
    pooled = torch.empty(groups, n, ho, wo, c, device=dev())
    argmax = torch.empty(groups, n, ho, wo, c, dtype=torch.uint8, device=dev())
    ops.bn_relu_maxpool_fwd(y_d, scale, shift, pooled, argmax, groups, n, h, w, c, ho, wo)
    gp = _rand(rng, groups, n, ho, wo, c, loc=0.2)
    # max-pool backward through argmax, in fp64
    am = argmax.cpu().numpy().astype(np.int64)
    gi, ni, oy, ox, ci = np.indices(am.shape)
    iy, ix = 2 * oy - 1 + am // 3, 2 * ox - 1 + am % 3
    dpix = np.zeros((groups, n, h, w, c))
    np.add.at(dpix, (gi, ni, iy, ix, ci), gp.astype(np.float64))
    sc, sh = scale.cpu().double().numpy(), shift.cpu().double().numpy()
    on = (y.astype(np.float64) * sc[:, None, None, None, :] + sh[:, None, None, None, :]) > 0
    dy_ref, dg_ref, db_ref = _eval_ref(dpix * on, y, gamma, rm, rv)
    dy = torch.full_like(y_d, float("nan"))
    dg0, db0 = _rand(rng, c), _rand(rng, c)
    dgamma, dbeta = _t(dg0), _t(db0)
    ops.bn_relu_maxpool_eval_bwd(_t(gp), argmax, y_d, scale, shift, _t(gamma), _t(rm), _t(rv), EPS, groups, n, h, w, c, ho, wo,
                                 dy, dgamma, dbeta, accumulate)
    torch.cuda.synchronize()
    assert not torch.isnan(dy).any(), "a pixel of dy was not written"
    rel_close(dy, dy_ref, KTOL, "dy")
    base_g, base_b = (dg0.astype(np.float64), db0.astype(np.float64)) if accumulate else (0.0, 0.0)
    rel_close(dgamma, base_g + dg_ref, KTOL, "dgamma")
    rel_close(dbeta, base_b + db_ref, KTOL, "dbeta")


# ------------------------------------------------------------------------------------------ the model vs the oracle
@pytest.mark.parametrize("img_grad", [True, False], ids=["dimg", "no_dimg"])
@pytest.mark.parametrize("depth,batch,hw,gtol", [(18, 4, 96, GTOL), (50, 2, 160, 2 * GTOL), (18, 2, 224, GTOL)])
def test_eval_backward_strict_against_oracle(depth, batch, hw, gtol, img_grad):
    """Every parameter gradient (and d img) of an eval-mode step against the fp64 oracle in eval mode
    (R.model_forward(..., training=False)) with the HIP forward's ReLU pattern imposed."""
    from oracle import restatement as R
    m, sdn = build(depth)
    m._debug_keep_tapes = True
    data = inputs(batch, hw, seed=99)
    if img_grad:
        data["img_0"].requires_grad_(True)
        data["img_1"].requires_grad_(True)
    data = m(data)
    masks = _captured_masks(m)
    loss = metrics()(data)
    loss.backward()
    sd, leaves = _oracle_leaves(sdn)
    inp = synth.make_inputs(batch, 2, 99, hw)
    img, hp, gt = (torch.from_numpy(inp[k]) for k in ("img", "head_pose", "gt_gaze"))
    od = {"img_0": img[:, 0].double().requires_grad_(True), "img_1": img[:, 1].double().requires_grad_(True),
          "rot_0": R.rotation_matrix_2d(hp[:, 0]).double(), "rot_1": R.rotation_matrix_2d(hp[:, 1]).double(),
          "gt_gaze": gt[:, 0], "gt_gaze_1": gt[:, 1]}
    od = R.model_forward(sd, od, depth, 3, False, masks)
    ol = R.iteration_loss(od)
    ol.backward()
    rel_close(loss, ol.item(), TOL, "loss")
    rel_close(data["pred_gaze"], od["pred_gaze"], TOL, "pred_gaze")
    errs = _grad_errors(m, leaves)
    assert len(errs) == len(leaves) - 2          # everything but the unused fc.weight / fc.bias
    assert errs[0][0] <= gtol, "worst gradients (max-norm relative error): " + ", ".join(f"{k} {e:.2e}" for e, k in errs[:8])
    if img_grad:
        rel_close(data["img_0"].grad, od["img_0"].grad, gtol, "grad img_0")
        rel_close(data["img_1"].grad, od["img_1"].grad, gtol, "grad img_1")
    else:
        assert data["img_0"].grad is None


MV_CASES = [(18, 3, 4, 64), (18, 4, 3, 64), (50, 3, 2, 96), (50, 4, 2, 64)]


@pytest.mark.parametrize("depth,V,B,hw", MV_CASES, ids=[f"r{d}_V{v}_B{b}_hw{h}" for d, v, b, h in MV_CASES])
def test_eval_backward_multiview_against_oracle(depth, V, B, hw):
    """forward_multiview with V = 3, 4 in eval mode against R.multiview_forward(..., training=False) with the masks imposed."""
    from oracle import restatement as R
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    from rot_mvgaze_amd.losses import MultiViewIterationLoss
    from rot_mvgaze_amd.model import MultiViewGaze
    m = MultiViewGaze(depth, 3)
    sdn = synth.make_state_dict(depth, 0, 3, perturb_bn=True)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sdn.items()})
    m.to(dev()).eval()
    m._debug_keep_tapes = True
    before = _buffers(m)
    inp = synth.make_inputs(B, V, 7, hw)
    img, hp, gt = (torch.from_numpy(inp[k]) for k in ("img", "head_pose", "gt_gaze"))
    rot_d = rotation_matrix_2d(hp.reshape(-1, 2).to(dev())).reshape(B, V, 3, 3)
    out = m.forward_multiview(img.to(dev()), rot_d)
    masks = _captured_masks(m, V)
    loss = MultiViewIterationLoss(rel_weight=0.01, reference_decay=1.0, iter_decay=0.5)(out, gt.to(dev()))
    loss.backward()
    _assert_buffers_equal(before, m)
    sd, leaves = _oracle_leaves(sdn)
    rot = R.rotation_matrix_2d(hp.reshape(-1, 2)).reshape(B, V, 3, 3).double()
    oo = R.multiview_forward(sd, img.double(), rot, depth, 3, False, masks)
    ol = R.multiview_loss(oo, gt, iter_decay=0.5, rel_weight=0.01, reference_decay=1.0)
    ol.backward()
    rel_close(loss, ol.item(), TOL, "loss")
    errs = _grad_errors(m, leaves)
    assert len(errs) == len(leaves) - 2
    assert errs[0][0] <= 2 * GTOL, "worst gradients (max-norm relative error): " + ", ".join(f"{k} {e:.2e}" for e, k in errs[:8])


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_eval_backward_variants_against_oracle(name):
    """All five constructor variants at R18 (B = 3, 64 px) against the oracle's eval-mode gradients.  The oracle imposes
    hidden-layer ReLU patterns on the default fusion block only; the rotation-matrix-encoding and shared-feature variants
    get the backbone's and the lifter's patterns."""
    from oracle import restatement as R
    from rot_mvgaze_amd.arch import Variant, backbone_spec
    kw = VARIANTS[name]
    var = Variant(**kw)
    m, sdn = build(18, **kw)
    m._debug_keep_tapes = True
    before = _buffers(m)
    data = m(inputs(3, 64))
    head_masks = not (var.encode_rotmat or var.share_feature)
    masks = _captured_masks(m, head=head_masks)
    loss = metrics()(data)
    loss.backward()
    _assert_buffers_equal(before, m)
    sd, leaves = _oracle_leaves(sdn)
    inp = synth.make_inputs(3, 2, 1234, 64)
    img, hp, gt = (torch.from_numpy(inp[k]) for k in ("img", "head_pose", "gt_gaze"))
    spec = backbone_spec(18)
    feats = [R.backbone_forward(sd, img[:, v].double(), spec, False, None, masks["backbone"][v]) for v in range(2)]
    lifted = [R.lift(sd, feats[v], masks["lift"][v]) for v in range(2)]
    od = {"gt_gaze": gt[:, 0], "gt_gaze_1": gt[:, 1]}
    od.update(R.fuse_pair(sd, 3, feats[0], feats[1], lifted[0], lifted[1], R.rotation_matrix_2d(hp[:, 0]).double(),
                          R.rotation_matrix_2d(hp[:, 1]).double(), masks if head_masks else None, var, False))
    ol = R.iteration_loss(od)
    ol.backward()
    rel_close(loss, ol.item(), TOL, "loss")
    rel_close(data["pred_gaze"], od["pred_gaze"], TOL, "pred_gaze")
    errs = _grad_errors(m, leaves)
    assert errs[0][0] <= GTOL, "worst gradients (max-norm relative error): " + ", ".join(f"{k} {e:.2e}" for e, k in errs[:8])


# ------------------------------------------------------------------------------------------ side effects, order, sync
@pytest.mark.parametrize("depth,variant", [(18, {}), (50, {}), (18, dict(share_feature=True))], ids=["r18", "r50", "r18_share_feature"])
def test_eval_backward_leaves_every_buffer_untouched(depth, variant):
    """Running mean / var, num_batches_tracked and the IntensityBatchNorm running_mean: bit-identical after an eval-mode
    forward + backward."""
    m, _ = build(depth, **variant)
    before = _buffers(m)
    assert any(k.endswith("num_batches_tracked") for k in before)
    if variant.get("share_feature"):
        assert any("_batchnorm.running_mean" in k for k in before)
    data = inputs(4, 64)
    data["img_0"].requires_grad_(True)
    loss = metrics()(m(data))
    loss.backward()
    torch.cuda.synchronize()
    _assert_buffers_equal(before, m)
    assert all(p.grad is not None for k, p in m.named_parameters() if ".fc." not in k)


def test_eval_backward_run_to_run_determinism():
    """The partial sums are added in a fixed order: two eval-mode backward passes give bit-identical loss and gradients."""
    m, _ = build(18)
    runs = []
    for _ in range(2):
        m.zero_grad(set_to_none=False)
        data = m(inputs(16, 224, seed=5))
        loss = metrics()(data)
        loss.backward()
        runs.append((loss.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}))
    assert torch.equal(runs[0][0], runs[1][0])
    assert len(runs[0][1]) > 50
    for k, g in runs[0][1].items():
        assert torch.equal(g, runs[1][1][k]), k


@pytest.mark.parametrize("depth", [18, 50])
def test_eval_backward_publishes_gradients_in_train_mode_order(depth):
    """The batches handed to _on_grads_ready (data-parallel buckets, the fused Adam) are the same sequence of parameters in
    eval mode as in train mode."""
    m, _ = build(depth)
    names = {id(p): k for k, p in m.named_parameters()}

    def batches(train):
        m.train(train)
        seen = []
        m._on_grads_ready = lambda ps: seen.append([names[id(p)] for p in ps])
        m.zero_grad(set_to_none=True)
        metrics()(m(inputs(2, 64))).backward()
        torch.cuda.synchronize()
        m._on_grads_ready = None
        return seen
    ev = batches(False)
    tr = batches(True)
    assert len(ev) > 5
    assert ev == tr


def test_eval_step_does_not_synchronise_the_host():
    """An eval-mode gradient step with the fused Adam, both APIs, under torch's sync debug mode."""
    from rot_mvgaze_amd.losses import MultiViewIterationLoss
    from rot_mvgaze_amd.optim import Adam
    m, _ = build(18)
    crit, crit_mv = metrics(), MultiViewIterationLoss(rel_weight=0.01, reference_decay=1.0, iter_decay=0.5)
    opt = Adam(m.parameters(), lr=1e-4, weight_decay=1e-6)
    d = inputs(4, 64)
    img = [d["img_0"], d["img_1"]]
    rot = torch.stack([d["rot_0"], d["rot_1"]], 1).contiguous()
    gt = torch.stack([d["gt_gaze"], d["gt_gaze_1"]], 1).contiguous()

    def step_dict():
        opt.zero_grad()
        crit(m(dict(d))).backward()
        opt.step()

    def step_mv():
        m.zero_grad(set_to_none=True)
        crit_mv(m.forward_multiview(img, rot), gt).backward()
        opt.step()
    for fn in (step_dict, step_mv):
        fn()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            fn()
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()


def test_eval_mode_fine_tuning_lowers_the_loss_and_keeps_the_statistics():
    """Person-specific calibration: three eval-mode Adam steps on one fixed batch lower the loss; BatchNorm statistics
    and the IntensityBatchNorm buffers stay frozen."""
    from rot_mvgaze_amd.optim import Adam
    m, _ = build(18)
    before = _buffers(m)
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
    _assert_buffers_equal(before, m)


def test_bf16_eval_backward_still_raises():
    m, _ = build(18)
    m.compute_dtype = torch.bfloat16
    loss = metrics()(m(inputs(2, 64)))
    with pytest.raises(NotImplementedError, match="bf16"):
        loss.backward()
