"""Range guard of the split path's backbone activations: every sp activation of a training step carries a per-tensor
power-of-two scale derived on the device from a parameter-only bound (tests/act_range_ref.py states it), so a layer with
a large or tiny BatchNorm gamma / beta - legal in a loaded checkpoint: the next BatchNorm undoes it in fp32 - neither
overflows fp16's range (NaN before this feature) nor loses small values absolutely.

Model level: the training step against the CPU oracle with the project's own bars (tests/test_model_gpu.py).  Kernel
level: the scaled BatchNorm apply / stem tail / average pool against float64 at the format's 2^-23 per element, and a conv
forward and weight gradient reading a scaled activation at the split kernels' bar (tests/test_split_gpu.py)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rot_mvgaze_amd  # noqa: F401
from act_range_ref import P, RANGE_CASES, RANGE_IDS, expected_sinv, modified_state_dict
from test_model_gpu import FTOL, TOL, dev, l2_bound, l2_close, rel_close

pytestmark = pytest.mark.gpu

SP_VS_F64 = 2e-7         # relative L2 of one stored sp tensor against float64: the format keeps 2^-23 per element (1.2e-7)
SPLIT_VS_F64 = 2e-6      # whole GEMMs on the split kernels (tests/test_split_gpu.py)
MAGS = [1e-6, 1e-3, 1.0, 1e3, 1e6]


def rel_l2(a, ref):
    return ((a.double() - ref).norm() / ref.norm()).item()


def pow2_sinv(bound):
    """2^-k that maps `bound` just below 2^15 (what a producer's scale does outside the dead band)."""
    _, e = math.frexp(float(bound))
    return 2.0 ** -(15 - e)


def slot(value):
    return torch.full((1,), float(value), dtype=torch.float32, device=dev())


def _mv_model(depth, sd):
    from rot_mvgaze_amd.model import MultiViewGaze
    m = MultiViewGaze(depth, 3)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    return m.to(dev()).train()


def _mv_inputs(B, V, hw, seed):
    from rot_mvgaze_amd import synth
    inp = synth.make_inputs(B, V, seed, hw)
    return tuple(torch.from_numpy(inp[k]) for k in ("img", "head_pose", "gt_gaze"))


# ---------------------------------------------------------------- model level
@pytest.mark.parametrize("depth,batch,hw,conditioned,bn,factor", RANGE_CASES, ids=RANGE_IDS)
def test_training_step_with_one_batchnorm_scaled_by_a_power_of_two(monkeypatch, depth, batch, hw, conditioned, bn, factor):
    """Forward, loss and backward on the split kernels against the oracle on the same modified state dict (V = 2).
    Before the activations carried a scale: NaN for every 2^16 / 2^20 case (the modified tensor overflows fp16), and
    1.2e-3 / 1.4e-3 on the pooled feature for the 2^-14 stem cases (CPU emulation of the storage format)."""
    from oracle import restatement as R
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    from rot_mvgaze_amd.losses import MultiViewIterationLoss
    monkeypatch.setenv("MVG_SPLIT", "1")
    V = 2
    sdn = modified_state_dict(depth, bn, factor, conditioned=conditioned)
    m = _mv_model(depth, sdn)
    img, hp, gt = _mv_inputs(batch, V, hw, 1234)
    rot_d = rotation_matrix_2d(hp.reshape(-1, 2).to(dev())).reshape(batch, V, 3, 3)
    out = m.forward_multiview([img[:, v].contiguous().to(dev()) for v in range(V)], rot_d)
    assert m._backbone._split_now
    want = expected_sinv(sdn, depth, batch, hw, hw)
    got = {k: float(v) for k, v in m._backbone._act_sinv.items()}
    assert got == dict(want)
    assert any(v != 1.0 for v in got.values())
    loss = MultiViewIterationLoss(rel_weight=0.01, reference_decay=1.0, iter_decay=0.5)(out, gt.to(dev()))
    loss.backward()

    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sd = {k: torch.from_numpy(np.array(v)) for k, v in sdn.items()}
    leaves = {k: v.requires_grad_(True) for k, v in sd.items() if v.dtype == torch.float32 and "running" not in k}
    rot = R.rotation_matrix_2d(hp.reshape(-1, 2)).reshape(batch, V, 3, 3)
    oo = R.multiview_forward(sd, img, rot, depth, 3, True)
    ol = R.multiview_loss(oo, gt, iter_decay=0.5, rel_weight=0.01, reference_decay=1.0)
    ol.backward()
    figures = [f"loss {loss.item():.6f} oracle {ol.item():.6f}"]
    for v in range(V):
        for name, g_, o_ in (("img_feat", out["img_feat"][v], oo["img_feat"][v]),
                             ("initial_rot_feat", out["initial_rot_feat"][v], oo["initial_rot_feat"][v])):
            o_ = o_.detach().reshape(g_.shape)
            figures.append(f"{name}[{v}] {float((g_.detach().cpu() - o_).abs().max() / o_.abs().max()):.2e}")
    print("\n".join(figures))
    rel_close(loss, ol.item(), TOL, "loss")
    for v in range(V):
        rel_close(out["img_feat"][v], oo["img_feat"][v].detach().numpy(), FTOL, f"pooled feature, view {v}")
        rel_close(out["initial_rot_feat"][v].reshape(batch, -1), oo["initial_rot_feat"][v].detach().reshape(batch, -1).numpy(), FTOL,
                  f"lifted feature, view {v}")
    for pr in R.view_pairs(V):
        for it in range(3):
            for k in ("feat_0", "feat_1", "pred_gaze_0", "pred_gaze_1"):
                rel_close(out["pairs"][pr][f"iter_{it}"][k], oo["pairs"][pr][f"iter_{it}"][k].detach().numpy(),
                          TOL if "pred" in k else FTOL, f"pair {pr} iter {it} {k}")
    n = 0
    worst = []
    for k, p in m.named_parameters():
        if leaves[k].grad is None:
            assert p.grad is None, k
            continue
        assert bool(torch.isfinite(p.grad).all()), f"grad {k} is not finite"
        g_dev = (p.grad.contiguous() if p.grad.dim() == 4 else p.grad).detach().cpu().double().numpy()
        g_ref = leaves[k].grad.double().numpy()
        worst.append((float(np.linalg.norm((g_dev - g_ref).ravel()) / (np.linalg.norm(g_ref.ravel()) + 1e-30)), k))
        n += 1
    worst.sort(reverse=True)
    print("worst gradients (relative L2): " + ", ".join(f"{k} {e:.2e}" for e, k in worst[:5]))
    for k, p in m.named_parameters():
        if leaves[k].grad is not None:
            l2_close(p.grad.contiguous() if p.grad.dim() == 4 else p.grad, leaves[k].grad.numpy(), l2_bound(depth, batch, hw), "grad " + k)
    assert n > 60


UNMODIFIED = [(18, 2, 64), (50, 2, 64), (18, 2, 224), (50, 2, 224)]


@pytest.mark.parametrize("depth,batch,hw", UNMODIFIED)
def test_slots_of_unmodified_networks_are_all_one(monkeypatch, depth, batch, hw):
    monkeypatch.setenv("MVG_SPLIT", "1")
    sdn = modified_state_dict(depth)
    m = _mv_model(depth, sdn)
    img, hp, _ = _mv_inputs(batch, 2, hw, 7)
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    rot_d = rotation_matrix_2d(hp.reshape(-1, 2).to(dev())).reshape(batch, 2, 3, 3)
    m.forward_multiview(img.to(dev()), rot_d)
    assert m._backbone._split_now
    got = {k: float(v) for k, v in m._backbone._act_sinv.items()}
    assert got == dict(expected_sinv(sdn, depth, batch, hw, hw))
    assert len(got) == {18: 17, 50: 49}[depth] and set(got.values()) == {1.0}


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_gamma_gives_scale_one(monkeypatch, bad):
    monkeypatch.setenv("MVG_SPLIT", "1")
    sdn = modified_state_dict(18)
    a = sdn[P + "layer2.0.bn1.weight"].copy()
    a[3] = bad
    sdn[P + "layer2.0.bn1.weight"] = a
    m = _mv_model(18, sdn)
    img, hp, _ = _mv_inputs(2, 2, 64, 7)
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    rot_d = rotation_matrix_2d(hp.reshape(-1, 2).to(dev())).reshape(2, 2, 3, 3)
    m.forward_multiview(img.to(dev()), rot_d)
    got = {k: float(v) for k, v in m._backbone._act_sinv.items()}
    assert got == dict(expected_sinv(sdn, 18, 2, 64, 64)) and set(got.values()) == {1.0}


def test_act_scales_kernel_on_a_hand_built_chain():
    """mvg_act_scales alone: records with and without a slot, a chain over three records, channel counts that are not a
    multiple of the wave size, against the fp32 expression evaluated on the host."""
    from rot_mvgaze_amd import ops
    from act_range_ref import sinv_for, unit_bound
    torch.manual_seed(5)
    cs, ns = [64, 7, 2048, 130, 256], [8, 1, 401408, 50, 3]
    mags = [1.0, 1e-5, 3.0, 1e7, 100.0]
    g = [(torch.randn(c) * mg).to(dev()) for c, mg in zip(cs, mags)]
    b = [(torch.randn(c) * mg * 0.1).to(dev()) for c, mg in zip(cs, mags)]
    ident, slots_of = [-1, -1, -1, 2, 3], [0, 1, -1, 2, 3]
    rec = [(g[i].data_ptr(), b[i].data_ptr(), cs[i], math.sqrt(max(ns[i] - 1, 0)), ident[i], slots_of[i]) for i in range(5)]
    items = np.array(rec, dtype=np.dtype([("gamma", "<i8"), ("beta", "<i8"), ("c", "<i4"), ("s", "<f4"), ("ident", "<i4"), ("slot", "<i4")]))
    table = torch.from_numpy(items.view("<i8").reshape(5, 4).copy()).to(dev())
    slots = torch.full((5,), float("nan"), device=dev())
    ops.act_scales(table, 5, slots)
    ub = [unit_bound(g[i].cpu().numpy(), b[i].cpu().numpy(), ns[i]) for i in range(5)]
    chain = list(ub)
    for i in range(5):
        if ident[i] >= 0:
            chain[i] = np.float32(ub[i] + chain[ident[i]])
    want = [sinv_for(chain[0]), sinv_for(chain[1]), sinv_for(chain[3]), sinv_for(chain[4])]
    got = slots.cpu().tolist()
    assert got[:4] == want and math.isnan(got[4])                  # the slot no record names is not written
    # a slot holds 2^-k: 1 in the band, below 1 for a tiny bound (stored times 2^k > 1), above 1 for a huge one and its chain
    assert want[0] == 1.0 and want[1] < 1.0 and want[2] > 1.0 and want[3] > 1.0


# ---------------------------------------------------------------- kernel level
def _old_bn_apply_split(y, scale, shift, residual, relu, out_sp, G, rows, c, raff=None, want_bits=False):
    """The unscaled entry point itself (ops.bn_apply_split goes through the scaled one)."""
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import check, lib
    bits = torch.empty(G * rows * c // 4, dtype=torch.uint8, device=y.device) if want_bits else None
    rs, rh = raff if raff is not None else (None, None)
    p = ops._p
    check(lib().mvg_bn_apply_split(p(y), p(scale), p(shift), p(residual), int(ops.is_sp(residual)), p(rs), p(rh), int(relu), p(out_sp),
                                   p(bits), G, rows, c, ops._s()), "bn_apply_split (unscaled entry point)")
    return bits


@pytest.mark.parametrize("mag", MAGS)
@pytest.mark.parametrize("res", [None, "sp", "raw"])
@pytest.mark.parametrize("relu", [True, False])
def test_scaled_bn_apply_against_float64(mag, res, relu):
    """The activation's magnitude goes through gamma / beta (scale, shift) and a matching sinv: merge_sp(out) against float64,
    the ReLU mask bits against the fp32 pass on the same values and against the unscaled call, and with sinv = 1 the bytes of
    the unscaled entry point."""
    from rot_mvgaze_amd import ops
    G, N, H, Cc = 2, 3, 9, 128
    rows = N * H * H
    torch.manual_seed(int(abs(math.log10(mag))) * 7 + (3 if res else 0) + relu)
    y = torch.randn(G, rows, Cc, device=dev()) * 2 + 0.5
    scale, shift = (torch.rand(G, Cc, device=dev()) + 0.5) * mag, torch.randn(G, Cc, device=dev()) * 0.3 * mag
    ref = y.double() * scale.double()[:, None] + shift.double()[:, None]
    rs = r32 = raff = None
    if res == "sp":                 # an sp identity with its OWN scale: four times the unit's magnitude
        r = torch.relu(torch.randn(G, rows, Cc, device=dev())) * (4 * mag)
        rsinv = pow2_sinv(float(r.abs().max()))
        rs = ops.split_f32(r, 1.0 / rsinv)
        if rs.sinv is None:
            rs.sinv = slot(1.0)
        r32 = ops.merge_sp(rs)          # the values the pass reads back (exact in fp32)
        ref = ref + r32.double()
    elif res == "raw":              # the raw downsample output with its affine
        rs = r32 = torch.randn(G, rows, Cc, device=dev())
        raff = ((torch.rand(G, Cc, device=dev()) + 0.5) * mag, torch.randn(G, Cc, device=dev()) * 0.2 * mag)
        ref = ref + (r32.double() * raff[0].double()[:, None] + raff[1].double()[:, None])
    if relu:
        ref = torch.relu(ref)
    out = ops.sp_empty(G, rows, Cc, device=dev())
    out.sinv = slot(pow2_sinv(float(ref.abs().max())))
    bits = ops.bn_apply_split(y, scale, shift, rs, relu, out, G, rows, Cc, raff, want_bits=True)
    assert float(out.float().abs().max()) < 65504.0
    err = rel_l2(ops.merge_sp(out), ref)
    print(f"bn_apply mag {mag:g} res {res} relu {relu}: {err:.2e}")
    assert err <= SP_VS_F64, f"{err:.2e}"
    # the mask bits are decided on the unscaled value: those of the fp32 pass on the same numbers ...
    if res:
        want = torch.empty_like(y)
        want_bits = ops.bn_apply_bits(y, scale, shift, r32, want, G, rows, Cc, raff)
        assert torch.equal(bits, want_bits)
    # ... and, on inputs the unscaled entry point can take (an sp identity without a scale), ITS bits whatever the output's
    # scale is (its stored pieces overflow at 1e6; its bits do not care), and with sinv = 1.0 its bytes
    ru = ops.split_f32(torch.relu(torch.randn(G, rows, Cc, device=dev()))) if res == "sp" else rs
    out_u = ops.sp_empty(G, rows, Cc, device=dev())
    bits_u = _old_bn_apply_split(y, scale, shift, ru, relu, out_u, G, rows, Cc, raff, want_bits=True)
    out_s = ops.sp_empty(G, rows, Cc, device=dev())
    out_s.sinv = slot(pow2_sinv(float(ref.abs().max())))
    assert torch.equal(ops.bn_apply_split(y, scale, shift, ru, relu, out_s, G, rows, Cc, raff, want_bits=True), bits_u)
    out_1 = ops.sp_empty(G, rows, Cc, device=dev())
    out_1.sinv = slot(1.0)
    if res == "sp":
        ru.sinv = slot(1.0)
    bits_1 = ops.bn_apply_split(y, scale, shift, ru, relu, out_1, G, rows, Cc, raff, want_bits=True)
    assert torch.equal(out_1.view(torch.int16), out_u.view(torch.int16)) and torch.equal(bits_1, bits_u)


@pytest.mark.parametrize("mag", MAGS)
def test_scaled_stem_tail_against_float64(mag):
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import check, lib
    G, N, H, Cc = 2, 3, 30, 64
    torch.manual_seed(3)
    y = torch.randn(G, N, H, H, Cc, device=dev())
    scale, shift = (torch.rand(G, Cc, device=dev()) + 0.5) * mag, torch.randn(G, Cc, device=dev()) * 0.3 * mag
    hp = (H + 2 - 3) // 2 + 1
    a = torch.relu(y.double() * scale.double()[:, None, None, None] + shift.double()[:, None, None, None])
    ref = F.max_pool2d(a.view(G * N, H, H, Cc).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).reshape(G, N, hp, hp, Cc)
    out, am = ops.sp_empty(G, N, hp, hp, Cc, device=dev()), torch.empty(G, N, hp, hp, Cc, dtype=torch.uint8, device=dev())
    out.sinv = slot(pow2_sinv(float(ref.abs().max())))
    ops.bn_relu_maxpool_fwd_split(y, scale, shift, out, am, G, N, H, H, Cc, hp, hp)
    assert float(out.float().abs().max()) < 65504.0
    err = rel_l2(ops.merge_sp(out), ref)
    print(f"stem tail mag {mag:g}: {err:.2e}")
    assert err <= SP_VS_F64, f"{err:.2e}"
    # the unscaled entry point: the same argmax always; with sinv = 1.0 the same bytes
    out_u, am_u = ops.sp_empty(G, N, hp, hp, Cc, device=dev()), torch.empty_like(am)
    p = ops._p
    check(lib().mvg_bn_relu_maxpool_fwd_split(p(y), p(scale), p(shift), p(out_u), p(am_u), G, N, H, H, Cc, hp, hp, ops._s()), "unscaled stem tail")
    assert torch.equal(am, am_u)
    out_1, am_1 = ops.sp_empty(G, N, hp, hp, Cc, device=dev()), torch.empty_like(am)
    out_1.sinv = slot(1.0)
    ops.bn_relu_maxpool_fwd_split(y, scale, shift, out_1, am_1, G, N, H, H, Cc, hp, hp)
    assert torch.equal(out_1.view(torch.int16), out_u.view(torch.int16)) and torch.equal(am_1, am_u)


@pytest.mark.parametrize("mag", MAGS)
def test_scaled_average_pool_against_float64(mag):
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import check, lib
    n, hw, Cc = 6, 49, 512
    torch.manual_seed(11)
    x = torch.relu(torch.randn(n, hw, Cc, device=dev()) + 0.3) * mag
    xs = ops.split_f32(x, 1.0 / pow2_sinv(float(x.abs().max())))
    if xs.sinv is None:
        xs.sinv = slot(1.0)
    ref = ops.merge_sp(xs).double().mean(dim=1)
    feat = torch.empty(n, Cc, device=dev())
    ops.avgpool_fwd_split(xs, feat, n, hw, Cc)
    err = rel_l2(feat, ref)
    print(f"average pool mag {mag:g}: {err:.2e}")
    assert err <= SP_VS_F64, f"{err:.2e}"
    # sinv = 1.0: the bytes of the unscaled entry point
    xu = ops.split_f32(torch.relu(torch.randn(n, hw, Cc, device=dev())))
    f_u, f_1 = torch.empty(n, Cc, device=dev()), torch.empty(n, Cc, device=dev())
    check(lib().mvg_avgpool_fwd_split(ops._p(xu), ops._p(f_u), n, hw, Cc, ops._s()), "unscaled average pool")
    xu.sinv = slot(1.0)
    ops.avgpool_fwd_split(xu, f_1, n, hw, Cc)
    assert torch.equal(f_1.view(torch.int32), f_u.view(torch.int32))


@pytest.mark.parametrize("mag", MAGS)
@pytest.mark.parametrize("case", [(2, 3, 14, 256, 256, 3, 1, 1), (1, 5, 28, 128, 128, 3, 2, 1), (2, 16, 14, 1024, 256, 1, 1, 0)],
                         ids=lambda c: "g%d_n%d_h%d_%dto%d_k%d_s%d" % c[:7])
def test_conv_forward_and_weight_gradient_read_a_scaled_activation(case, mag):
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import ConvDesc
    G, N, h, cin, cout, k, st, pad = case
    torch.manual_seed(sum(case))
    d = ConvDesc.make(G, N, h, h, cin, cout, k, st, pad)
    x = torch.relu(torch.randn(G, N, h, h, cin, device=dev())) * mag
    w = torch.randn(cout, k, k, cin, device=dev()) * (1.0 / (k * k * cin) ** 0.5)
    gy = torch.randn(G, N, d.ho, d.wo, cout, device=dev()) * 2.0 ** -20
    xs = ops.split_f32(x, 1.0 / pow2_sinv(float(x.abs().max())))
    gys = ops.split_f32(gy, 2.0 ** 28)
    wk, _ = ops.split_weights(d, w, False)
    xr = x.double().view(G * N, h, h, cin).permute(0, 3, 1, 2)
    wr = w.double().permute(0, 3, 1, 2).requires_grad_(True)
    yr = F.conv2d(xr, wr, None, st, pad)
    yr.backward(gy.double().view(G * N, d.ho, d.wo, cout).permute(0, 3, 1, 2))
    y_ref = yr.detach().permute(0, 2, 3, 1).reshape(G, N, d.ho, d.wo, cout)
    dw_ref = wr.grad.permute(0, 2, 3, 1)
    y = torch.empty(G, N, d.ho, d.wo, cout, device=dev())
    ops.conv_fprop_split(d, xs, wk, y, None)
    dw = torch.empty_like(w)
    ops.conv_wgrad_split(d, xs, gys, dw)
    # the deferred form: slabs now, their sums in one launch (when the shape splits its pixels at all)
    dw2, defer = torch.empty_like(w), []
    ops.conv_wgrad_split(d, xs, gys, dw2, False, defer=defer)
    if defer:
        ops.wgrad_reduce_batch(defer)
    e_y, e_w, e_w2 = rel_l2(y, y_ref), rel_l2(dw, dw_ref), rel_l2(dw2, dw_ref)
    print(f"conv reading a scaled activation, mag {mag:g}: fprop {e_y:.2e} wgrad {e_w:.2e} deferred {e_w2:.2e}")
    assert e_y <= SPLIT_VS_F64 and e_w <= SPLIT_VS_F64 and e_w2 <= SPLIT_VS_F64


def test_scaled_entry_points_reject_what_they_do_not_cover():
    """A null required pointer and c % 8 != 0: a non-zero code and a message, no launch."""
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import ConvDesc, lib
    L, p, s = lib(), ops._p, ops._s
    f = torch.zeros(4096, device=dev())
    u8 = torch.zeros(4096, dtype=torch.uint8, device=dev())
    h16 = torch.zeros(8192, dtype=torch.float16, device=dev())
    d = ConvDesc.make(1, 2, 4, 4, 32, 32, 1, 1, 0)

    def rejected(rc, text):
        msg = L.mvg_last_error()
        assert rc != 0 and msg and text in msg.decode(), (rc, msg)
    rejected(L.mvg_bn_apply_split_scaled(None, p(f), p(f), None, 0, None, None, None, 1, p(h16), p(f), None, 1, 4, 16, s()), "required")
    rejected(L.mvg_bn_apply_split_scaled(p(f), p(f), p(f), None, 0, None, None, None, 1, None, p(f), None, 1, 4, 16, s()), "required")
    rejected(L.mvg_bn_apply_split_scaled(p(f), p(f), p(f), None, 0, None, None, None, 1, p(h16), p(f), None, 1, 4, 12, s()), "c % 8")
    rejected(L.mvg_bn_apply_split_scaled(p(f), p(f), p(f), p(f), 0, None, None, p(f), 1, p(h16), p(f), None, 1, 4, 16, s()), "res_sinv")
    rejected(L.mvg_bn_relu_maxpool_fwd_split_scaled(p(f), p(f), p(f), None, p(f), p(u8), 1, 1, 4, 4, 16, 2, 2, s()), "required")
    rejected(L.mvg_bn_relu_maxpool_fwd_split_scaled(p(f), p(f), p(f), p(h16), p(f), p(u8), 1, 1, 4, 4, 12, 2, 2, s()), "c % 8")
    rejected(L.mvg_avgpool_fwd_split_scaled(None, p(f), p(f), 2, 4, 16, s()), "required")
    rejected(L.mvg_avgpool_fwd_split_scaled(p(h16), p(f), p(f), 2, 4, 12, s()), "c % 8")
    rejected(L.mvg_conv_wgrad_split_xs(C.byref(d), None, p(f), p(h16), p(f), p(f), None, 1, 0, s()), "required")
    rejected(L.mvg_conv_wgrad_split_slabs_xs(C.byref(d), p(h16), p(f), None, p(f), p(f), 2, s()), "required")
    rejected(L.mvg_conv_wgrad_split_slabs_xs(C.byref(d), p(h16), p(f), p(h16), p(f), None, 2, s()), "workspace")
    rejected(L.mvg_act_scales(None, 1, p(f), 1, s()), "required")
    rejected(L.mvg_act_scales(p(f), 0, p(f), 1, s()), "records")
    rejected(L.mvg_act_scales(p(f), 257, p(f), 1, s()), "records")
    torch.cuda.synchronize()
