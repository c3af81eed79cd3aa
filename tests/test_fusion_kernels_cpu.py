"""No GPU: (1) the float64 references of tests/fusion_kernels_ref.py against something independent - the operand builders, the
IntensityBatchNorm walk and their backward against the oracle's fusers (oracle/restatement.py: the tensors R.fuse / R.fuse_rotmat /
R.fuse_rotfeat / R.gaze_head hand their Mlp, the running_mean R.intensity_batchnorm leaves, and autograd through them) for
V = 2 and for V = 3 as a loop of R.fuse_pair over R.view_pairs(3) on one shared state dict; the losses against R.multiview_loss
and the reference's fixtures; the max-pool argmax code against a scan written out in Python; (2) the preconditions of the case
tables tests/test_fusion_kernels_gpu.py runs, on the references alone, so that a GPU failure cannot be an ill-conditioned input;
(3) the launchers' rejection messages (MVG_REQUIRE returns before any launch: the library needs no device for them)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rot_mvgaze_amd  # noqa: F401
from oracle import restatement as R
from rot_mvgaze_amd._lib import lib
from rot_mvgaze_amd.arch import Variant

import fusion_kernels_ref as ref
from fusion_kernels_ref import NVEC

I3 = 3          # iterations


def rel_err(got, want):
    return float((got.double() - want.double()).abs().max()) / (float(want.double().abs().max()) + 1e-300)


# ---------------------------------------------------------------- (1) the references against the oracle
def _oracle_run(monkeypatch, variant, V, B, training, cf=512):
    """R.fuse_pair over every pair on one shared state dict with R.mlp replaced by a tap: it records the tensor each fuser / head
    Mlp is fed and answers with a fresh random leaf (so every iteration's features are known tensors that take a gradient)."""
    inp = ref.rotcat_inputs(V, B, cf)
    # float64 rotations, orthonormal to 1e-16: the norm of a rotated column (what the oracle's normaliser sees) is then the column's
    # (what the kernel and ref.ibn_scales read); rounded to float32 they are orthonormal to ~6e-8, which moves the scales by as much
    inp["rot"] = ref.rotations(B * V, 11, torch.float64).view(B, V, 3, 3)
    img = [inp["img"][v].double().requires_grad_(True) for v in range(V)]
    lifted = [inp["lifted"][v].double().requires_grad_(True) for v in range(V)]
    rot = inp["rot"].double()
    rm0 = [0.5 + ref.rand((NVEC,), 70 + it).double() for it in range(I3)]
    sd = {f"_img_fusers.{it}._batchnorm.running_mean": rm0[it].view(1, 1, -1).clone() for it in range(I3)}
    calls = []

    def tap(sd_, prefix, x, n_layers, relu_masks=None):
        y = ref.randn((x.shape[0], 2 if prefix.startswith("_gaze") else 3 * NVEC), 1000 + len(calls)).double().requires_grad_(True)
        calls.append((prefix, n_layers, x, y))
        return y
    monkeypatch.setattr(R, "mlp", tap)
    for (i, j) in R.view_pairs(V):
        R.fuse_pair(sd, I3, img[i], img[j], lifted[i], lifted[j], rot[:, i], rot[:, j], None, variant, training)
    D = inp["D"]
    assert len(calls) == (D // 2) * I3 * 4
    X = [[None] * D for _ in range(I3)]
    Fo = [[None] * D for _ in range(I3)]
    H = [[None] * D for _ in range(I3)]
    for p in range(D // 2):
        for it in range(I3):
            base = (p * I3 + it) * 4
            for s in (0, 1):
                pre, nl, x, y = calls[base + s]
                assert pre == f"_img_fusers.{it}._fuser." and nl == (3 if variant.encode_rotmat or variant.share_feature else 2)
                X[it][2 * p + s], Fo[it][2 * p + s] = x, y
                pre, nl, x, _ = calls[base + 2 + s]
                assert pre == f"_gaze_estimators.{it}." and nl == 2
                H[it][2 * p + s] = x
    return inp, img, lifted, sd, rm0, X, Fo, H


VARIANTS = {"default": {}, "ignore_rotmat": {"ignore_rotmat": True}, "encode_rotmat": {"encode_rotmat": True},
            "share_feature": {"share_feature": True}}


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("V", [2, 3])
@pytest.mark.parametrize("name", list(VARIANTS))
def test_builders_reproduce_what_the_oracle_feeds_its_mlps_and_its_autograd(monkeypatch, name, V, training):
    v = Variant(**VARIANTS[name])
    B, cf = 4, 512
    inp, img, lifted, sd, rm0, X, Fo, H = _oracle_run(monkeypatch, v, V, B, training, cf)
    vi, vj, D, rel = inp["vi"], inp["vj"], inp["D"], inp["rel"].double()
    rel64 = ref.relative_rotation(inp["rot"], vi, vj)
    partner, ident = [d ^ 1 for d in range(D)], list(range(D))
    img_t, lift_t = torch.stack(img).detach(), torch.stack(lifted).detach()
    feats = [torch.stack(Fo[it]).detach().view(D, B, 3, NVEC) for it in range(I3)]
    a = lift_t if v.share_feature else img_t
    scales = [None] * I3
    kin = X[0][0].shape[-1]
    for it in range(I3):
        src, src_of = (lift_t, vj) if it == 0 else (feats[it - 1], partner)
        got = torch.stack(X[it]).detach()
        if v.share_feature:
            scales[it], rm = ref.ibn_scales(a, src, vi, src_of, rm0[it], training)
            want = ref.paircat(a, src, rel64, scales[it], vi, src_of)
            assert rel_err(sd[f"_img_fusers.{it}._batchnorm.running_mean"].reshape(-1), rm) <= 1e-13
            if not training:
                assert torch.equal(rm, rm0[it])
            want_h = ref.paircat(a, feats[it], None, None, vi, ident)
        elif v.encode_rotmat:
            want = ref.rotcat_ext(img_t, src, None, rel64, vi, src_of, kin)
            padded = ref.rotcat_ext(img_t, src, None, rel64, vi, src_of, kin + 3)
            assert kin == cf + 3 * NVEC + 9 and torch.equal(padded[..., :kin], want) and float(padded[..., kin:].abs().max()) == 0.0
            want_h = ref.rotcat(img_t, feats[it], None, vi, ident)
        else:
            want = ref.rotcat(img_t, src, None if v.ignore_rotmat else rel64, vi, src_of)
            want_h = ref.rotcat(img_t, feats[it], None, vi, ident)
        assert got.shape == want.shape and rel_err(got, want) <= 1e-13, (name, it)
        assert rel_err(torch.stack(H[it]).detach(), want_h) <= 1e-13, (name, it)
    # ---- backward: a random gradient on every Mlp input, autograd through the oracle's builders against the references
    GX = [ref.randn((D, B, kin), 300 + it).double() for it in range(I3)]
    GH = [ref.randn((D, B, H[0][0].shape[-1]), 400 + it).double() for it in range(I3)]
    total = 0.0
    for it in range(I3):
        total = total + (torch.stack(X[it]) * GX[it]).sum() + (torch.stack(H[it]) * GH[it]).sum()
    total.backward()
    rel_f = None if (v.ignore_rotmat or v.encode_rotmat) else rel64
    aw = 3 * NVEC if v.share_feature else cf
    da = torch.zeros(V, B, aw, dtype=torch.float64)
    dlift = None
    for it in range(I3):
        # the head input of this iteration and the fuser input of the next one both read feats[it]
        if v.share_feature:
            da_h, dF = ref.paircat_bwd(GH[it], None, None, ident, D)
            da = ref.segment_sum(da_h.flatten(-2, -1), aw, vi, V, da)
            da_x, dsrc = ref.paircat_bwd(GX[it], rel_f, scales[it], partner if it else ident, D)
            da = ref.segment_sum(da_x.flatten(-2, -1), aw, vi, V, da)
        else:
            dF = ref.rotcat_bwd(GH[it], None, ident, D, cf)
            da = ref.segment_sum(GH[it], cf, vi, V, da)
            bwd = ref.rotcat_ext_bwd if v.encode_rotmat else ref.rotcat_bwd
            dsrc = bwd(GX[it], rel_f, partner if it else ident, D, cf)
            da = ref.segment_sum(GX[it], cf, vi, V, da)
        if it == 0:
            dlift = ref.segment_sum(dsrc.flatten(-2, -1), 3 * NVEC, vj, V)
        else:
            dprev = dprev + dsrc                                  # feats[it - 1]: its head's and this fuser's terms
            got = torch.stack([f.grad for f in Fo[it - 1]]).view(D, B, 3, NVEC)
            assert rel_err(got, dprev) <= 1e-12, (name, it)
        dprev = dF
    assert rel_err(torch.stack([f.grad for f in Fo[I3 - 1]]).view(D, B, 3, NVEC), dprev) <= 1e-12
    got_lift = torch.stack([t.grad for t in lifted]).view(V, B, -1)
    if v.share_feature:
        assert rel_err(got_lift, dlift + da) <= 1e-12
        assert all(t.grad is None for t in img)
    else:
        assert rel_err(got_lift, dlift) <= 1e-12
        assert rel_err(torch.stack([t.grad for t in img]), da) <= 1e-12
    assert float((rel - rel64).abs().max()) <= 1e-7          # (the float32 rel the GPU cases use is this one, rounded)
    ortho = rel.float().double() @ rel.float().double().transpose(-1, -2) - torch.eye(3, dtype=torch.float64)
    assert float(ortho.abs().max()) <= 3e-7


def test_ibn_walk_moves_the_buffer_before_it_divides_and_clamps_with_eps():
    """Hand-computed: one direction, one column, batch of two norms 3 and 5 (variance 1) then a constant column (variance 0)."""
    a = torch.zeros(1, 2, 3, 1)
    a[0, 0, 0, 0], a[0, 1, 1, 0] = 3.0, 5.0
    feat = torch.zeros(1, 2, 3, 1)
    feat[0, :, 2, 0] = 2.0
    s, rm = ref.ibn_scales(a, feat, [0], [0], torch.tensor([1.0]), True, 0.05, 1e-4)
    rm1 = 0.95 * 1.0 + 0.05 * 1.0
    rm2 = 0.95 * rm1 + 0.05 * 1e-2                              # sqrt(max(0, eps)) = 0.01
    assert abs(float(s[0, 0]) - 1 / (rm1 + 1e-4)) < 1e-15 and abs(float(s[1, 0]) - 1 / (rm2 + 1e-4)) < 1e-15 and abs(float(rm) - rm2) < 1e-15
    s, rm = ref.ibn_scales(a, feat, [0], [0], torch.tensor([1.0]), False, 0.05, 1e-4)
    assert float(rm) == 1.0 and float((s - 1 / 1.0001).abs().max()) < 1e-15


def test_skinny_and_segment_sum_references_are_autograd_and_index_add():
    x, w, b, dy = ref.randn((7, 10), 1), ref.randn((3, 10), 2), ref.randn((3,), 3), ref.randn((7, 3), 4)
    xr, wr, br = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    y = F.linear(F.relu(xr), wr, br)
    assert torch.equal(ref.skinny_fwd(F.relu(x), w, b), y.detach())
    y.backward(dy.double())
    dw0, db0 = ref.randn((3, 10), 5), ref.randn((3,), 6)
    dx, dw, db = ref.skinny_bwd(dy, F.relu(x), w, F.relu(x), dw0, db0)
    assert rel_err(dx, xr.grad) <= 1e-14 and rel_err(dw, wr.grad + dw0.double()) <= 1e-14 and rel_err(db, br.grad + db0.double()) <= 1e-14
    assert rel_err(ref.skinny_bwd(dy, x, w, None)[0], dy.double() @ w.double()) <= 1e-14
    g = ref.randn((6, 2, 12), 7)
    seg = [0, 2, 2, 0, 0, 2]
    want = torch.zeros(4, 2, 8, dtype=torch.float64).index_add_(0, torch.tensor(seg), g.double()[..., :8])
    got = ref.segment_sum(g, 8, seg, 4)
    assert torch.equal(got, want) and float(got[1].abs().max()) == 0.0 and float(got[3].abs().max()) == 0.0
    assert torch.equal(ref.segment_sum(g, 8, seg, 4, torch.ones(4, 2, 8)), want + 1)


def test_loss_references_reproduce_the_oracle_and_the_fixtures(golden_dir):
    V, B, rel_weight, ref_decay, iter_decay = 3, 5, 0.01, 0.7, 0.5
    vi, _ = ref.directed_pairs(V)
    D, npairs = len(vi), len(vi) // 2
    gt = (ref.rand((B, V, 2), 1) - 0.5)
    gt_dir = torch.stack([gt[:, v] for v in vi], 0).reshape(D * B, 2)
    pred = (gt_dir[None] + 0.3 * ref.randn((I3, D * B, 2), 2)).double().requires_grad_(True)
    out = {"pairs": {}}
    for p, (i, j) in enumerate(R.view_pairs(V)):
        pd = {"num_iter": I3}
        for it in range(I3):
            pd[f"iter_{it}"] = {f"pred_gaze_{s}": pred[it].view(D, B, 2)[2 * p + s] for s in (0, 1)}
        out["pairs"][(i, j)] = pd
    want = R.multiview_loss(out, gt.double(), iter_decay, rel_weight, ref_decay)
    want.backward()
    # the weights as losses.MultiViewIterationLoss forms them
    iw = [iter_decay ** (I3 - 1 - i) for i in range(I3)]
    dw = [(rel_weight if d % 2 == 0 else rel_weight * ref_decay) / npairs for d in range(D)]
    loss, dpred = ref.angular_loss_multi(pred.detach(), gt_dir, [iw[it] * dw[d] for it in range(I3) for d in range(D)], D, B)
    # (the oracle's pitchyaw_to_vector is float32, as the reference's: 1e-5 / 1e-4 are the project's bars for such a comparison)
    assert abs(float(loss) - float(want.detach())) <= 1e-5 * abs(float(want.detach()))
    assert float((dpred - pred.grad).abs().max()) <= 1e-4 * float(pred.grad.abs().max())
    # ... and one iteration, one direction of it is angular_loss with the row weight w / batch
    th, l1, d1 = ref.angular_loss(pred.detach()[1, 2 * B:3 * B], gt_dir[2 * B:3 * B], iw[1] * dw[2] / B)
    assert rel_err(d1, dpred[1, 2 * B:3 * B]) <= 1e-12 and abs(float(l1) - float(th.sum()) * iw[1] * dw[2] / B) <= 1e-15
    g = np.load(os.path.join(golden_dir, "geometry_loss.npz"))
    p32, g32 = torch.from_numpy(g["loss_pred"]), torch.from_numpy(g["loss_gt"])
    th, l, d = ref.angular_loss(p32, g32, 1.0 / p32.shape[0])
    np.testing.assert_allclose(float(l), g["loss"], rtol=1e-5)
    # the fixture's gradient is the reference's float32 autograd: comparable to 1e-4 on the rows where 1 / sqrt(1 - sim^2) does not
    # amplify float32 rounding (angle >= 0.1 rad, the precondition of the GPU cases); a coincident row has gradient exactly 0 in both
    ok = (th / ref.DEG >= 0.1).numpy()
    assert ok.sum() >= 16
    np.testing.assert_allclose(d.numpy()[ok], g["loss_dpred"][ok], rtol=1e-4, atol=1e-4 * np.abs(g["loss_dpred"]).max())
    assert all(float(np.abs(g["loss_dpred"][i]).max()) == 0.0 for i in np.nonzero(np.abs(d.numpy()).max(1) == 0.0)[0])
    np.testing.assert_allclose(th.numpy(), R.angular_error_numpy(p32.numpy().astype(np.float64), g32.numpy().astype(np.float64)), rtol=1e-9)
    g = np.load(os.path.join(golden_dir, "lp_loss.npz"))
    for p, lt in ((1, "l1"), (2, "l2")):
        l, d = ref.lp_loss(torch.from_numpy(g["pred"]), torch.from_numpy(g["label"]), p)
        np.testing.assert_allclose(float(l), g[f"{lt}_loss"], rtol=1e-6)
        np.testing.assert_allclose(d.numpy(), g[f"{lt}_dpred"], rtol=1e-6, atol=1e-9)
        assert float(d[3].abs().max()) == 0.0                   # pred == label there


def test_maxpool_reference_code_is_the_first_maximum_in_scan_order():
    n, h, w, c = 2, 5, 6, 3
    x = ref.maxpool_input(n, h, w, c)
    y, code, _ = ref.maxpool(x)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    assert tuple(code.shape) == (n, ho, wo, c) and ref.maxpool_tie_fraction(x) > 0.25
    for ni in range(n):
        for ci in range(c):
            for oy in range(ho):
                for ox in range(wo):
                    best, k = None, None
                    for kh in range(3):
                        for kw in range(3):
                            iy, ix = oy * 2 - 1 + kh, ox * 2 - 1 + kw
                            if 0 <= iy < h and 0 <= ix < w and (best is None or float(x[ni, ci, iy, ix]) > best):
                                best, k = float(x[ni, ci, iy, ix]), kh * 3 + kw
                    assert int(code[ni, oy, ox, ci]) == k and float(y[ni, oy, ox, ci]) == best
    gy = ref.randn((n, c, ho, wo), 3)
    dx = ref.maxpool(x, gy)[2]
    want = torch.zeros(n, h, w, c, dtype=torch.float64)
    for ni in range(n):
        for ci in range(c):
            for oy in range(ho):
                for ox in range(wo):
                    k = int(code[ni, oy, ox, ci])
                    want[ni, oy * 2 - 1 + k // 3, ox * 2 - 1 + k % 3, ci] += float(gy[ni, ci, oy, ox])
    assert torch.equal(dx, want)
    z = ref.randn((3, 4, 8), 1)
    assert rel_err(ref.avgpool(z), F.adaptive_avg_pool1d(z.double().transpose(1, 2), 1)[..., 0]) <= 1e-15
    assert torch.equal(ref.avgpool_bwd(ref.avgpool(z), 4)[:, 2], ref.avgpool(z) / 4)


# ---------------------------------------------------------------- (2) preconditions of the case tables
def test_ibn_cases_keep_every_column_variance_away_from_eps_on_both_sides():
    eps = ref.IBN_EPS
    seen_b, seen_v, seen_tr = set(), set(), set()
    for (V, B, tr, kind) in ref.IBN_CASES:
        c = ref.ibn_inputs(V, B, kind)
        var = ref.ibn_call_variances(c["a"], c["feat"], c["vi"], c["src_of"])
        assert var.shape == (2 * c["D"], NVEC)
        assert not bool(((var >= eps / 2) & (var <= 2 * eps)).any()), (V, B)
        clamped = var < eps / 2
        cl = torch.arange(NVEC) % ref.IBN_CLAMPED_EVERY == 0
        if B == 1:
            assert bool(clamped.all())
        else:
            assert bool(clamped[:, cl].all()) and bool((var[:, ~cl] > 2 * eps).all()), (V, B)
        # the walk is order-sensitive on these inputs: the scales of two consecutive calls differ (training, B > 1)
        if tr and B > 1:
            s, rm = ref.ibn_scales(c["a"], c["feat"], c["vi"], c["src_of"], c["rm"], True)
            assert float((s[1:] / s[:-1] - 1).abs().median()) > 1e-3 and float((rm / c["rm"].double() - 1).abs().median()) > 1e-2
        seen_b.add(B), seen_v.add(2 * c["D"]), seen_tr.add(tr)
    assert seen_b == {1, 5, 33} and seen_v == {4, 12, 24} and seen_tr == {True, False}
    assert len({k for (_, _, _, k) in ref.IBN_CASES}) == 2


def test_float32_cost_of_the_ibn_walk_sets_its_bar():
    """ref.IBN_SCALES_BAR is four times the error of the walk done in float32 on the CPU against the float64 reference - a figure of
    the number format, taken without any kernel; the plain builders' 1e-6 is below it at 24 calls."""
    mom, eps = float(np.float32(ref.IBN_MOMENTUM)), float(np.float32(ref.IBN_EPS))
    worst = {}
    for (V, B, tr, kind) in ref.IBN_CASES:
        if not tr:
            continue
        c = ref.ibn_inputs(V, B, kind)
        s64, rm64 = ref.ibn_scales(c["a"], c["feat"], c["vi"], c["src_of"], c["rm"], True, mom, eps)
        s32, rm32 = ref.ibn_scales_f32(c["a"], c["feat"], c["vi"], c["src_of"], c["rm"], mom, eps)
        worst[c["D"]] = max(worst.get(c["D"], 0.0), rel_err(s32, s64))
        assert rel_err(rm32, rm64) <= 1e-6                       # the buffer itself stays within the builders' bar
    print("float32 walk vs float64, max error over max scale, per D:", worst)
    assert worst[2] < worst[6] < worst[12] and 1e-6 < worst[12] <= ref.IBN_SCALES_BAR / 4 * 1.001


def test_angular_cases_stay_where_the_gradient_is_well_conditioned():
    for n in ref.ANGULAR_NS:
        pred, gt = ref.angular_inputs(n)
        th = ref.angles(pred.double(), gt.double()) / ref.DEG
        assert float(th.min()) >= 0.1 and float(th.max()) <= 1.0, n
        assert float(pred[:, 0].abs().max()) < 1.2 and float(gt[:, 0].abs().max()) < 1.2
    for (iters, dirs, batch) in ref.ANGULAR_MULTI_CASES:
        assert iters * dirs <= 512
        pred, gt = ref.angular_multi_inputs(iters, dirs, batch)
        assert pred.shape == (iters, dirs * batch, 2)
        th = ref.angles(pred.double(), gt.double()[None].expand_as(pred)) / ref.DEG
        assert float(th.min()) >= 0.1 and float(th.max()) <= 1.0 and float(pred[..., 0].abs().max()) < 1.2
    assert (1, 512, 1) in ref.ANGULAR_MULTI_CASES and set(ref.ANGULAR_NS) >= {1, 255, 257}


def test_maxpool_cases_are_full_of_ties():
    for (n, h, w, c) in ref.MAXPOOL_CASES:
        x = ref.maxpool_input(n, h, w, c)
        assert float(x.min()) >= 0.0 and c % 4 == 0
        if h * w > 1:                                            # (a 1 x 1 image has one-element windows: nothing to tie)
            assert ref.maxpool_tie_fraction(x) >= 0.25, (n, h, w, c)
            assert float((x == 0).double().mean()) > 0.3


def test_shape_tables_reach_the_edges_they_are_for():
    assert any(cf // 4 > 256 for (_, _, cf, _, _) in ref.ROTCAT_CASES) and {V for (V, *_) in ref.ROTCAT_CASES} == {3, 4}
    for (V, B, cf, ld, ap, ad) in ref.ROTCAT_EXT_CASES:
        assert ld % 4 == 0 and ld >= cf + 3 * NVEC + 9
    assert (3, 5, 512, 2060, False, True) in ref.ROTCAT_EXT_CASES and any(ld - (cf + 3 * NVEC) > 256 + 9 for (_, _, cf, ld, _, _) in ref.ROTCAT_EXT_CASES)
    assert len({(ap, ad) for (_, _, _, _, ap, ad) in ref.ROTCAT_EXT_CASES}) == 4
    for (V, B, cf, segs, acc) in ref.SEGSUM_CASES:
        assert segs == V + 1                                    # segment V is empty
    assert any((segs * B * cf // 4) % 256 for (_, B, cf, segs, _) in ref.SEGSUM_CASES) and {acc for (*_, acc) in ref.SEGSUM_CASES} == {True, False}
    assert max(ref.STREAM_NS) > 4096 * 256 and {1, 255, 257} <= set(ref.STREAM_NS)
    big = [r * k for (r, k, _) in ref.SKINNY_CASES if r * k > 1024 * 256]
    assert big and {o for (_, _, o) in ref.SKINNY_CASES} == {1, 2, 3, 4} and any(k % 4 for (_, k, _) in ref.SKINNY_CASES)
    assert any((n * c // 4) % 256 for (n, _, c) in ref.AVGPOOL_CASES) and {hw for (_, hw, _) in ref.AVGPOOL_CASES} == {1, 4, 49}


# ---------------------------------------------------------------- (3) rejections
def _last_error():
    msg = lib().mvg_last_error()
    return msg.decode() if msg else ""


def _rejected(rc, text):
    assert rc != 0 and text in _last_error(), (rc, _last_error())


def test_launchers_reject_bad_sizes_with_a_message():
    L = lib()
    buf = (C.c_float * 1024)()                                  # a non-null address for the checks that want one (never read)
    q = C.addressof(buf)
    # nvec % 4: the rows of cf + 3 nvec floats move as 16-byte vectors
    _rejected(L.mvg_rotcat_fwd(None, None, None, None, None, None, 2, 2, 512, 511, None), "rotcat: nvec % 4 != 0")
    _rejected(L.mvg_rotcat_fwd(None, None, None, None, None, None, 2, 2, 510, 512, None), "rotcat: cf % 4 != 0")
    _rejected(L.mvg_rotcat_bwd(None, None, None, None, 2, 2, 512, 510, None), "rotcat_bwd: nvec % 4 != 0")
    _rejected(L.mvg_rotcat_ext_fwd(None, None, None, None, None, None, None, 2060, 2, 2, 512, 510, None), "rotcat_ext: nvec % 4 != 0")
    _rejected(L.mvg_rotcat_ext_bwd(None, 2060, None, None, None, 2, 2, 512, 510, None), "rotcat_ext_bwd: nvec % 4 != 0")
    _rejected(L.mvg_paircat_fwd(None, None, None, None, None, None, None, 2, 2, 511, None), "paircat: nvec % 4 != 0")
    _rejected(L.mvg_paircat_bwd(None, None, None, None, None, None, 2, 2, 513, None), "paircat_bwd: nvec % 4 != 0")
    _rejected(L.mvg_fuse_unbuild(q, None, None, q, q, q, q, 0, 2, 2, 2, 2, 512, 511, None, None), "fuse_unbuild: nvec % 4 != 0")
    _rejected(L.mvg_fuse_unbuild(q, None, None, q, q, q, q, 0, 2, 2, 2, 0, 512, 512, None, None), "fuse_unbuild: bad sizes")
    # batch > 0 and dirs > 0
    for batch, dirs in ((0, 2), (2, 0), (-1, 2)):
        _rejected(L.mvg_relative_rotation(None, None, None, None, batch, 3, dirs, None), "relative_rotation: batch, views and dirs must be positive")
        _rejected(L.mvg_rotcat_fwd(None, None, None, None, None, None, batch, dirs, 512, 512, None), "rotcat: batch and dirs must be positive")
        _rejected(L.mvg_rotcat_bwd(None, None, None, None, batch, dirs, 512, 512, None), "rotcat_bwd: batch and dirs must be positive")
        _rejected(L.mvg_rotcat_ext_fwd(None, None, None, None, None, None, None, 2060, batch, dirs, 512, 512, None),
                  "rotcat_ext: batch and dirs must be positive")
        _rejected(L.mvg_rotcat_ext_bwd(None, 2060, None, None, None, batch, dirs, 512, 512, None), "rotcat_ext_bwd: batch and dirs must be positive")
        _rejected(L.mvg_paircat_fwd(None, None, None, None, None, None, None, batch, dirs, 512, None), "paircat: batch and dirs must be positive")
        _rejected(L.mvg_paircat_bwd(None, None, None, None, None, None, batch, dirs, 512, None), "paircat_bwd: batch and dirs must be positive")
        _rejected(L.mvg_segment_sum(None, 2048, 512, None, None, batch, dirs, 2, 0, None), "segment_sum: batch, dirs, segments and width must be positive")
        _rejected(L.mvg_ibn_scales(None, None, None, None, None, 1, 0.05, 1e-4, None, batch, dirs, 512, None), "ibn_scales: bad sizes")
    # the messages that were there
    _rejected(L.mvg_ibn_scales(None, None, None, None, None, 1, 0.05, 1e-4, None, 2, 2, 0, None), "ibn_scales: bad sizes")
    _rejected(L.mvg_segment_sum(None, 2048, 510, None, None, 2, 2, 2, 0, None), "segment_sum: width/row_stride % 4 != 0")
    _rejected(L.mvg_segment_sum(None, 2050, 512, None, None, 2, 2, 2, 0, None), "segment_sum: width/row_stride % 4 != 0")
    for nout in (0, 5):
        _rejected(L.mvg_linear_skinny_fwd(None, None, None, None, 4, 8, nout, None), "skinny linear: out_features must be 1..4")
        _rejected(L.mvg_linear_skinny_bwd(None, None, None, None, None, None, None, 4, 8, nout, 0, None, None), "skinny linear: out_features must be 1..4")
    _rejected(L.mvg_gaze_lp_loss(None, None, 8, 3, None, None, None), "gaze_lp_loss: n > 0 and p in {1, 2}")
    _rejected(L.mvg_gaze_lp_loss(None, None, 0, 1, None, None, None), "gaze_lp_loss: n > 0 and p in {1, 2}")
    _rejected(L.mvg_gaze_angular_loss(None, None, 0, 1.0, None, 0, None, None, None), "gaze loss: n <= 0")
    w = (C.c_float * 513)()
    _rejected(L.mvg_gaze_angular_loss_multi(q, q, 27, 19, 1, w, q, None, None), "gaze_angular_loss_multi: bad arguments (iters * dirs <= 512)")
    _rejected(L.mvg_gaze_angular_loss_multi(q, q, 1, 513, 1, w, q, None, None), "gaze_angular_loss_multi: bad arguments (iters * dirs <= 512)")
    _rejected(L.mvg_rotcat_ext_fwd(None, None, None, q, None, None, None, 2056, 2, 2, 512, 512, None), "rotcat_ext: ld too small")
    _rejected(L.mvg_rotcat_ext_fwd(None, None, None, None, None, None, None, 2044, 2, 2, 512, 512, None), "rotcat_ext: ld too small")
    _rejected(L.mvg_rotcat_ext_fwd(None, None, None, q, None, None, None, 2058, 2, 2, 512, 512, None), "rotcat_ext: cf / ld % 4 != 0")
    _rejected(L.mvg_rotcat_ext_bwd(None, 2058, None, None, None, 2, 2, 512, 512, None), "rotcat_ext_bwd: cf / ld % 4 != 0")
    _rejected(L.mvg_rotcat_ext_bwd(None, 2044, None, None, None, 2, 2, 512, 512, None), "rotcat_ext_bwd: ld too small")
    _rejected(L.mvg_maxpool3x3s2_fwd(None, None, None, 1, 4, 4, 6, 2, 2, None), "maxpool: c % 4 != 0")
    _rejected(L.mvg_maxpool3x3s2_fwd(None, None, None, 1, 4, 4, 8, 3, 2, None), "maxpool: bad output size")
    _rejected(L.mvg_avgpool_fwd(None, None, 1, 4, 6, None), "avgpool: c % 4 != 0")
