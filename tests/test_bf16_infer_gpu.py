"""The bf16 storage path's inference form (model.compute_dtype = torch.bfloat16 under model.eval() + torch.no_grad()).

What runs: per conv + BatchNorm unit ONE launch, mvg_conv_fprop_bf16_affine,

    out = bf16( [relu]( acc * scale[c] + shift[c] [+ residual] ) )

acc = the fp32 accumulator, scale / shift the BatchNorm's running statistics as a per-channel affine, the ReLU after the
add, one rounding at the store; the stem keeps conv -> fused BatchNorm + ReLU + max pool; raw uint8 patches go straight to
the stem's bf16 NHWC8 input; the bf16 weight copies stay between calls while the parameters are unchanged.

Tolerances are the ones tests/test_bf16_gpu.py declares.  OUT_RTOL = 6e-3: a bf16-rounded output against float64, max-norm
relative to max |reference| - half an ulp of bf16 is 2^-9 = 2e-3, so float64 arithmetic rounded once stays inside it by
construction, and the fp32 accumulation error (K <= 4608 products, ~1e-6 relative) does not show at that scale.
BF16_VS_FP32_SANITY = 0.6: the end-to-end sanity bound of the random-initialised networks.  The float64 references are
written here (torch on the CPU)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd import synth

pytestmark = pytest.mark.gpu

OUT_RTOL = 6e-3
BF16_VS_FP32_SANITY = 0.6
BN_EPS = 1e-5
IMAGE_MEAN, IMAGE_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def dev():
    return torch.device("cuda:0")


def rnd(shape, seed, tag="t", scale=1.0):
    n = int(np.prod(shape))
    return torch.from_numpy((synth.normal(n, seed, tag) * scale).astype(np.float32).reshape(shape))


def bf(x):
    return x.to(torch.bfloat16)


def rel_err(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return (got - ref).abs().max().item() / (ref.abs().max().item() + 1e-30)


def close(got, ref, rtol, what=""):
    e = rel_err(got, ref)
    print(f"[bf16 infer] {what}: rel {e:.3e} (bound {rtol:.1e})")
    assert e <= rtol, f"{what}: max err relative to max |ref| {e:.3e} > {rtol:.1e}"


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def to_nhwc(x):     # [G,N,C,H,W] -> [G,N,H,W,C]
    return x.permute(0, 1, 3, 4, 2).contiguous()


# the shapes of tests/test_bf16_gpu.py: both kernel forms (LDS-DMA for 64-channel taps, register-staged for the stem's 8-channel
# and the 32-channel taps), both tile widths, stride 2, ragged last tiles
BF16_CONV_CASES = [
    # G, N, H, W, Cin, Cout, k, stride, pad
    (2, 3, 14, 14, 64, 128, 3, 1, 1),
    (2, 3, 15, 13, 64, 128, 3, 2, 1),
    (1, 5, 14, 14, 128, 64, 1, 1, 0),
    (2, 2, 14, 14, 64, 256, 1, 2, 0),
    (2, 2, 36, 36, 8, 64, 7, 2, 3),
    (2, 8, 56, 56, 64, 256, 1, 1, 0),
    (1, 16, 28, 28, 128, 128, 3, 1, 1),
    (2, 2, 7, 7, 512, 512, 3, 1, 1),
    (2, 4, 16, 16, 64, 128, 3, 2, 1),
    (1, 2, 28, 28, 256, 512, 1, 2, 0),
    (1, 30, 14, 14, 256, 256, 3, 1, 1),
    (1, 3, 9, 9, 32, 32, 3, 1, 1),
    (2, 16, 56, 56, 64, 64, 3, 1, 1),
]


@pytest.mark.parametrize("case", BF16_CONV_CASES)
def test_conv_fprop_bf16_affine(case):
    """mvg_conv_fprop_bf16_affine against float64: conv of the same bf16-rounded x, w, then * scale + shift (+ residual), ReLU,
    for {no residual, residual} x {relu, no relu}; scale has both signs and zeros.  And with scale = 1, shift = 0, no
    residual, no ReLU it equals mvg_conv_fprop_bf16 element for element (same accumulators, same single rounding)."""
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import ConvDesc
    G, N, H, W, Cin, Cout, k, st, pad = case
    x = bf(rnd((G, N, Cin, H, W), 1, "x")).float()
    stem = Cin == 8 and k == 7
    if stem:
        x[:, :, 3:] = 0
    cin_src = 3 if stem else Cin
    w = rnd((Cout, cin_src, k, k), 2, "w", 1.0 / np.sqrt(cin_src * k * k))
    d = ConvDesc.make(G, N, H, W, Cin, Cout, k, st, pad)
    acc = F.conv2d(x.reshape(G * N, Cin, H, W)[:, :cin_src].double(), bf(w).double(), None, st, pad)
    acc = acc.reshape(G, N, Cout, d.ho, d.wo).permute(0, 1, 3, 4, 2)                    # [G, N, ho, wo, Cout] float64
    scale = rnd((Cout,), 11, "scale")
    scale[::7] = 0.0
    assert float(scale.min()) < 0 < float(scale.max())
    shift = rnd((Cout,), 12, "shift", 0.5)
    res = bf(rnd((G, N, d.ho, d.wo, Cout), 13, "res"))

    xd = bf(to_nhwc(x)).to(dev())
    wk, _ = ops.cast_weights_bf16(d, w.permute(0, 2, 3, 1).contiguous().to(dev()), cin_src, False)
    scale_d, shift_d, res_d = scale.to(dev()), shift.to(dev()), res.to(dev())
    for with_res in (False, True):
        for relu in (False, True):
            out = torch.full((G, N, d.ho, d.wo, Cout), float("nan"), dtype=torch.bfloat16, device=dev())
            ops.conv_fprop_bf16_affine(d, xd, wk, out, scale_d, shift_d, res_d if with_res else None, relu)
            ref = acc * scale.double() + shift.double()
            if with_res:
                ref = ref + res.double()
            if relu:
                ref = F.relu(ref)
            close(out, ref, OUT_RTOL, f"affine {case} residual={with_res} relu={relu}")
    if not res_d.equal(res.to(dev())):
        raise AssertionError("the residual was written")
    plain = torch.empty(G, N, d.ho, d.wo, Cout, dtype=torch.bfloat16, device=dev())
    ops.conv_fprop(d, xd, wk, plain, None, False, None)
    ident = torch.empty_like(plain)
    ops.conv_fprop_bf16_affine(d, xd, wk, ident, torch.ones(Cout, device=dev()), torch.zeros(Cout, device=dev()), None, False)
    assert torch.equal(ident, plain), "scale 1 / shift 0 must reproduce mvg_conv_fprop_bf16"


RESIZE_CASES = [(2, 37, 41, 24), (1, 100, 90, 64), (1, 50, 60, 96), (1, 96, 96, 48), (1, 64, 64, 64)]   # n, h, w, size (resize_aa.npz)


def _preprocess_pair(u8, size, swap):
    """(the new kernel's bf16 NHWC8 output, the existing fp32 kernel's output converted and zero-padded to 8 channels)"""
    from rot_mvgaze_amd import ops
    n, h, w, _ = u8.shape
    src = torch.from_numpy(np.ascontiguousarray(u8)).to(dev())
    want32 = torch.empty(n, size, size, 4, device=dev())
    ops.preprocess_u8hwc_resize(src, want32, n, h, w, size, size, IMAGE_MEAN, IMAGE_STD, swap)
    want = torch.zeros(n, size, size, 8, dtype=torch.bfloat16, device=dev())
    want[..., :4] = want32.to(torch.bfloat16)
    got = torch.full((n, size, size, 8), float("nan"), dtype=torch.bfloat16, device=dev())
    ops.preprocess_u8hwc_resize_bf16(src, got, n, h, w, size, size, IMAGE_MEAN, IMAGE_STD, swap)
    return got, want


def test_preprocess_u8_to_bf16_nhwc8_bit_for_bit(golden_dir):
    """mvg_preprocess_u8hwc_resize_bf16 equals the existing fp32 kernel's output converted with .to(bfloat16) and zero-padded to
    8 channels, bit for bit, on the shapes test_kernels_gpu.py uses (resizes up and down, h == oh && w == ow, BGR swap)."""
    g = np.load(os.path.join(golden_dir, "resize_aa.npz"))
    n_cases = 0
    for idx, (n, h, w, size) in enumerate(RESIZE_CASES):
        for swap in (False, True):
            got, want = _preprocess_pair(g[f"u8_{idx}"], size, swap)
            assert bits_equal(got, want), f"case {idx} swap={swap}"
            n_cases += 1
    rng = np.random.default_rng(5)
    for (h, w) in ((256, 240), (180, 200), (224, 224)):
        u8 = rng.integers(0, 256, size=(2, h, w, 3), dtype=np.uint8)
        for swap in (False, True):
            got, want = _preprocess_pair(u8, 224, swap)
            assert bits_equal(got, want), f"{h}x{w} swap={swap}"
            assert float(got[..., 3:].float().abs().max()) == 0.0
            n_cases += 1
    assert n_cases == 16


# ---------------------------------------------------------------------------------------------- model level
def _model(depth, sdn=None, seed=0):
    from rot_mvgaze_amd.model import MultiViewGaze
    m = MultiViewGaze(depth, 3)
    if sdn is None:
        sdn = synth.make_state_dict(depth, seed, 3, perturb_bn=True)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sdn.items()})
    m.to(dev()).eval()
    m.compute_dtype = torch.bfloat16
    return m


def _inputs(B, V, hw, seed=5):
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    inp = synth.make_inputs(B, V, seed, hw)
    img, hp = torch.from_numpy(inp["img"]), torch.from_numpy(inp["head_pose"])
    rot_d = rotation_matrix_2d(hp.reshape(-1, 2).to(dev())).reshape(B, V, 3, 3)
    return img, hp, [img[:, v].contiguous().to(dev()) for v in range(V)], rot_d


@pytest.mark.parametrize("depth,n_convs", [(18, 20), (50, 53)])
def test_inference_launch_structure_and_kept_weight_copies(depth, n_convs):
    """One conv launch per unit and no BatchNorm apply pass; a second call with unchanged weights casts nothing (its layout
    family holds the V image repacks only) and returns the same bits."""
    from rot_mvgaze_amd import ops
    V, B, hw = 2, 2, 64
    m = _model(depth)
    _, _, imgs, _ = _inputs(B, V, hw)
    m.ensure_layout()
    bb = m._backbone
    bb.act_dtype = torch.bfloat16
    assert sum(1 for _ in bb.spec.all_convs()) == n_convs
    outs, profs = [], []
    ops.prof_enable(True)
    try:
        for call in range(2):
            ops.prof_reset()
            with torch.no_grad():
                feat, tape = bb.forward(imgs, training=False, keep_tape=False)
            torch.cuda.synchronize()
            profs.append(ops.prof_collect())
            outs.append(feat.clone())
            assert tape is None
    finally:
        ops.prof_enable(False)
    for pr in profs:
        assert pr.get("bn_apply", {"launches": 0})["launches"] == 0, pr
        assert pr["conv_fprop"]["launches"] == n_convs, pr
    assert profs[0]["layout"]["launches"] == V + 1, profs[0]          # V image repacks + one batched weight cast
    assert profs[1]["layout"]["launches"] == V, profs[1]              # ... and no cast on the second call
    assert torch.equal(outs[0], outs[1])
    assert torch.isfinite(outs[0]).all()


def _preds(m, imgs, rot_d):
    with torch.no_grad():
        out = m.forward_multiview(imgs, rot_d)
    return out["_mvg_preds"].clone(), out["img_feat"].clone()


@pytest.mark.parametrize("pname", ["_feat_extractor.0.layer2.0.conv1.weight", "_img_fusers.0._fuser.blocks.0.0.weight"])
def test_kept_weight_copies_follow_the_weights(pname):
    """After p.data.mul_(2) + invalidate_weight_cache(), and after load_state_dict, the output is that of a fresh model built with
    those weights, bit for bit - for a conv weight (backbone copies) and a Linear weight (the head's copies)."""
    depth, V, B, hw = 18, 2, 2, 64
    sdn = synth.make_state_dict(depth, 0, 3, perturb_bn=True)
    _, _, imgs, rot_d = _inputs(B, V, hw)
    m = _model(depth, sdn)
    p0, f0 = _preds(m, imgs, rot_d)
    p0b, _ = _preds(m, imgs, rot_d)                       # served from the kept copies
    assert torch.equal(p0, p0b)
    # a write that bypasses the version counter, then the documented call
    dict(m.named_parameters())[pname].data.mul_(2)
    m.invalidate_weight_cache()
    p1, f1 = _preds(m, imgs, rot_d)
    sd2 = {k: np.array(v) for k, v in sdn.items()}
    sd2[pname] = sd2[pname] * np.float32(2)
    fresh = _model(depth, sd2)
    p1f, f1f = _preds(fresh, imgs, rot_d)
    assert torch.equal(p1, p1f) and torch.equal(f1, f1f)
    assert not torch.equal(p1, p0), "doubling a weight must change the output"
    # load_state_dict moves the version counters: no call needed
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sdn.items()})
    p2, f2 = _preds(m, imgs, rot_d)
    fresh0 = _model(depth, sdn)
    p2f, f2f = _preds(fresh0, imgs, rot_d)
    assert torch.equal(p2, p2f) and torch.equal(f2, f2f)
    assert torch.equal(p2, p0)


def _check_units_teacher_forced(m, recs, img_feat):
    """Every recorded unit from ITS OWN recorded bf16 input (and residual): float64 conv + eval affine (+ residual) + ReLU must
    reproduce the recorded output; the stem's y, its pooled map and the final average pool likewise."""
    P = m._named_tensors()
    specs = {c.name: c for c in m._backbone.spec.all_convs()}
    no_relu = {blk.downsample.name for blk in m._backbone.spec.blocks if blk.downsample is not None}
    n_checked = 0
    for name, x, second, out in recs:
        c = specs[name]
        G, N, H, W, _ = x.shape
        xin = x.float().cpu().double().reshape(G * N, H, W, -1).permute(0, 3, 1, 2)[:, :c.cin]
        w = bf(P[c.name + ".weight"].detach().float().cpu().contiguous()).double()
        acc = F.conv2d(xin, w, None, c.stride, c.pad)
        gamma, beta = P[c.bn + ".weight"].detach().cpu().double(), P[c.bn + ".bias"].detach().cpu().double()
        rm, rv = P[c.bn + ".running_mean"].cpu().double(), P[c.bn + ".running_var"].cpu().double()
        scale = gamma / torch.sqrt(rv + BN_EPS)
        shift = beta - rm * scale
        nchw = lambda t: t.float().cpu().double().reshape(G * N, t.shape[2], t.shape[3], c.cout).permute(0, 3, 1, 2)
        if c.cin == 3:                                                  # stem: (input, raw y, pooled map)
            y_got = nchw(second)
            close(y_got, acc, OUT_RTOL, f"{name}: conv output y")
            act = F.relu(y_got * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))        # from the stored (rounded) y, as the kernel does
            close(nchw(out), F.max_pool2d(act, 3, 2, 1), OUT_RTOL, f"{name}: pooled activation")
        else:
            ref = acc * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
            if second is not None:
                ref = ref + nchw(second)
            if name not in no_relu:           # every unit but the downsample branch ends in a ReLU (BasicBlock / Bottleneck)
                ref = F.relu(ref)
            close(nchw(out), ref, OUT_RTOL, f"{name}: output" + (" (+ residual)" if second is not None else ""))
        n_checked += 1
    last = recs[-1][3]
    G, N = last.shape[0], last.shape[1]
    close(img_feat, last.float().cpu().reshape(G, N, -1, last.shape[-1]).mean(2), 1e-5, "average pool")
    return n_checked


TEACHER_CASES = [(18, 64), (50, 64), (50, 224)]


@pytest.mark.parametrize("depth,hw", TEACHER_CASES)
def test_inference_units_teacher_forced(depth, hw):
    from rot_mvgaze_amd.backbone import Backbone
    V, B = 2, 2
    m = _model(depth)
    _, _, imgs, rot_d = _inputs(B, V, hw)
    m.ensure_layout()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    bb = m._backbone
    assert Backbone._debug_units is None
    bb._debug_units = []
    try:
        with torch.no_grad():
            out = m.forward_multiview(imgs, rot_d)
        recs = bb._debug_units
    finally:
        bb._debug_units = None
    n_convs = sum(1 for _ in bb.spec.all_convs())
    assert len(recs) == n_convs == (20 if depth == 18 else 53)
    assert len({r[0] for r in recs}) == n_convs
    n_res = sum(1 for r in recs if r[0] != bb.spec.stem.name and r[2] is not None)
    assert n_res == len(bb.spec.blocks)                                   # every block's last unit took a residual
    assert _check_units_teacher_forced(m, recs, out["img_feat"]) == n_convs


@pytest.mark.parametrize("depth", [18, 50])
def test_inference_end_to_end_against_switch_off_and_fp32_oracle(depth):
    """(a) folded, (b) switch off = the parent's launches, (c) the fp32 oracle.  (a) vs (c) and (a) vs (b) on the predictions are
    sanity-bounded (the random-initialised networks amplify single roundings: see tests/test_bf16_gpu.py); the three distances
    are reported through MVG_TEST_L2_LOG."""
    from oracle import restatement as R
    V, B, hw = 2, 2, 64
    sdn = synth.make_state_dict(depth, 0, 3, perturb_bn=True)
    img, hp, imgs, rot_d = _inputs(B, V, hw)
    m = _model(depth, sdn)
    pa, _ = _preds(m, imgs, rot_d)
    m._backbone.bf16_fold_eval = False
    pb, _ = _preds(m, imgs, rot_d)
    m._backbone.bf16_fold_eval = True
    pa2, _ = _preds(m, imgs, rot_d)
    assert torch.equal(pa, pa2)                                           # the switch leaves no state behind
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    rot = R.rotation_matrix_2d(hp.reshape(-1, 2)).reshape(B, V, 3, 3)
    with torch.no_grad():
        o32 = R.multiview_forward({k: torch.from_numpy(np.array(v)) for k, v in sdn.items()}, img, rot, depth, 3, False)
    pc = torch.stack([torch.stack([o32["pairs"][pr][f"iter_{it}"][k] for pr in R.view_pairs(V) for k in ("pred_gaze_0", "pred_gaze_1")])
                      for it in range(3)])                                  # [I, D, B, 2] like _mvg_preds
    assert pc.shape == pa.shape
    d_ac, d_ab, d_bc = rel_err(pa, pc), rel_err(pa, pb), rel_err(pb, pc)
    log = os.environ.get("MVG_TEST_L2_LOG")
    tag = f"bf16-eval[r{depth}_V{V}_B{B}_hw{hw}]"
    lines = [f"{d_ac:.3e} {BF16_VS_FP32_SANITY:.1e} {tag} pred folded vs fp32 oracle",
             f"{d_ab:.3e} {BF16_VS_FP32_SANITY:.1e} {tag} pred folded vs switch-off",
             f"{d_bc:.3e} {BF16_VS_FP32_SANITY:.1e} {tag} pred switch-off vs fp32 oracle [reported]"]
    print("\n".join(lines))
    if log:
        with open(log, "a") as f:
            f.write("\n".join(lines) + "\n")
    assert d_ac <= BF16_VS_FP32_SANITY, f"folded vs fp32 oracle: {d_ac:.3e}"
    assert d_ab <= BF16_VS_FP32_SANITY, f"folded vs switch-off: {d_ab:.3e}"


@pytest.mark.parametrize("hin,win,size,bgr", [(64, 64, None, False), (80, 72, 64, False), (72, 90, 64, True)])
def test_uint8_patches_equal_the_fp32_preprocessed_input(hin, win, size, bgr):
    """Raw uint8 [B, H, W, 3] patches under no_grad equal, bit for bit, the same model fed the fp32 NCHW tensor that the fp32
    preprocessing kernel produces (both run the NHWC8 stem; the repack rounds the same values once)."""
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    depth, V, B = 18, 2, 3
    m = _model(depth)
    m.input_size, m.input_bgr = size, bgr
    rng = np.random.default_rng(17)
    u8 = [torch.from_numpy(rng.integers(0, 256, size=(B, hin, win, 3), dtype=np.uint8)).to(dev()) for _ in range(V)]
    hp = torch.from_numpy(synth.make_inputs(B, V, 5, 8)["head_pose"])
    rot_d = rotation_matrix_2d(hp.reshape(-1, 2).to(dev())).reshape(B, V, 3, 3)
    oh, ow = (size, size) if size else (hin, win)
    f32 = []
    for t in u8:
        nhwc4 = torch.empty(B, oh, ow, 4, device=dev())
        ops.preprocess_u8hwc_resize(t, nhwc4, B, hin, win, oh, ow, IMAGE_MEAN, IMAGE_STD, bgr)
        f32.append(nhwc4[..., :3].permute(0, 3, 1, 2).contiguous())
    p_raw, f_raw = _preds(m, u8, rot_d)
    p_f32, f_f32 = _preds(m, f32, rot_d)
    assert torch.isfinite(p_raw).all()
    assert torch.equal(f_raw, f_f32) and torch.equal(p_raw, p_f32)
    m.train()                                             # training steps keep the fp32 NCHW input
    with pytest.raises(NotImplementedError, match="inference only"):
        m.forward_multiview(u8, rot_d)
