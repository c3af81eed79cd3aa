"""Every small kernel of csrc/fusion.hip and csrc/pool.hip called directly (ops.*) against the float64 references of
tests/fusion_kernels_ref.py, at the smallest shapes that reach each edge (the tables of that module; their preconditions and the
references themselves are checked without a GPU in tests/test_fusion_kernels_cpu.py), and the constructor variants that keep the
materialised fp32 fusion path (encode_rotmat, share_feature) through FusionHead at V = 3 and 4 views.  Runs on an MI355X only.

Outputs and scratch start as NaN; every comparison asserts the output finite, prints
    FUSION-KERNELS <kernel> <case>: rel-L2 ... max-rel ...
(max-rel = max |got - want| / max |want|, what the bars bound) and then asserts.  The bars are the project's, not fitted:
  BUILD  1e-6   operand builders, segment_sum, axpby, scale_by, pools (test_rotcat_and_relative_rotation, test_bf16_gpu.py)
  RTOL   2e-5   the skinny Linear's products and sums (test_kernels_gpu.RTOL)
  loss   1e-5 relative on the value, 1e-4 relative + 1e-4 max |want| per element on the gradient (test_geometry_and_loss_golden)
  theta  1e-5 of the largest angle (the value bar, per row: angles >= 0.1 rad keep acos away from its steep end)
  head   2e-5 relative L2 (test_split_fusion_path_covers_the_variants_and_view_counts), running_mean 1e-6
One bar is not the project's: ibn_scales' scales are held to ref.IBN_SCALES_BAR = 4.4e-6, four times what the same walk in float32
costs in torch on the CPU (1.10e-6 at 24 calls, tests/test_fusion_kernels_cpu.py) - the first run had the kernel at 1.099e-6 there,
the CPU's float32 figure to four digits, over the 1e-6 that a 2-call walk meets easily.
Measured on an MI355X (every line: profiles/fusion_kernels_errors.txt), smallest .. largest max-rel per kernel, next to its bar:
  relative_rotation               5.1e-08 .. 5.4e-08   1e-6        rotcat_fwd / bwd                0 .. 1.2e-07 / 7.5e-08   1e-6
  rotcat_ext_fwd / bwd            0 .. 7.2e-08 / 7.3e-08   1e-6    paircat_fwd / bwd.da / .dfeat   0 .. 1.3e-07 / 5.4e-08 / 1.1e-07   1e-6
  ibn_scales (scales)             5.4e-08 .. 1.1e-06   4.4e-6      ibn_scales running_mean         2.3e-07 .. 4.9e-07   1e-6
  segment_sum                     0 .. 7.0e-08   1e-6              axpby / scale_by                1.2e-08 .. 7.0e-08 / 4.4e-08   1e-6
  linear_skinny fwd / dx          4.9e-08 .. 1.2e-07 / 1.0e-07   2e-5      linear_skinny dw / db   0 .. 2.7e-07 / 2.3e-07   2e-5
  gaze_angular_loss value         5.2e-08 .. 2.8e-07   1e-5        theta / gradient                3.9e-08 .. 1.2e-06 / 1.7e-06   1e-5 / 1e-4
  gaze_angular_loss_multi value   0 .. 3.2e-07   1e-5              gradient                        0 .. 1.4e-06   1e-4 (vs single launches: 1e-6)
  gaze_lp_loss value / gradient   0 .. 3.5e-08 / 0 .. 5.6e-08   1e-5 / 1e-4         rotation_matrix_2d   5.7e-08 .. 8.9e-08   1e-6
  maxpool_fwd / argmax / bwd      0 (equal to ATen's) / 0 differ / 0 .. 4.8e-08   1e-6
  avgpool_fwd / bwd               0 .. 3.3e-07 / 6.4e-08   1e-6    layout round trip               bit-equal
  head (rel-L2), V = 3 and 4      encode_rotmat 3.6e-07 .. 8.9e-07, share_feature 5.3e-07 .. 9.3e-07, share_weights + encode_rotmat
                                  3.5e-07 .. 3.7e-07   2e-5;   share_feature running_mean 4.0e-07 .. 8.6e-07   1e-6
The coincident rows (pred == gt): largest theta and gradient printed with the run, bound 0.1 degree."""
import math

import numpy as np
import pytest
import torch

import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd import ops

import fusion_kernels_ref as ref
from fusion_kernels_ref import NVEC
from test_kernels_gpu import RTOL, dev

pytestmark = pytest.mark.gpu

BUILD = 1e-6
LOSS_RTOL, GRAD_RTOL = 1e-5, 1e-4
MOM, EPS = float(np.float32(ref.IBN_MOMENTUM)), float(np.float32(ref.IBN_EPS))      # the values the C ABI's float arguments carry

def nan(*shape, dtype=torch.float32):
    if dtype == torch.uint8:
        return torch.full(shape, 255, dtype=dtype, device=dev())
    return torch.full(shape, float("nan"), dtype=dtype, device=dev())


def i32(a):
    return torch.tensor(list(a), dtype=torch.int32, device=dev())


def measure(kernel, case, got, want):
    got, want = got.detach().cpu().double().reshape(-1), want.detach().cpu().double().reshape(-1)
    assert got.shape == want.shape, (kernel, case, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f"{kernel} {case}: output not finite (unwritten or NaN)"
    diff = got - want
    l2 = float(diff.norm()) / (float(want.norm()) + 1e-300)
    mx = float(diff.abs().max()) / (float(want.abs().max()) + 1e-300)
    print(f"FUSION-KERNELS {kernel} {case}: rel-L2 {l2:.3e} max-rel {mx:.3e}")
    return l2, mx, diff, want


def hold(kernel, case, got, want, bar):
    l2, mx, _, _ = measure(kernel, case, got, want)
    assert mx <= bar, f"{kernel} {case}: max-rel {mx:.3e} > {bar:.1e}"


def hold_grad(kernel, case, got, want):
    """|got - want| <= 1e-4 |want| + 1e-4 max |want| at every element (assert_allclose's rule with the project's loss-gradient bars)."""
    _, _, diff, w = measure(kernel, case, got, want)
    over = diff.abs() - (GRAD_RTOL * w.abs() + GRAD_RTOL * float(w.abs().max()))
    assert float(over.max()) <= 0.0, f"{kernel} {case}: gradient off by {float(diff.abs().max()):.3e} (max |want| {float(w.abs().max()):.3e})"


def hold_value(kernel, case, got, want):
    got, want = float(got), float(want)
    assert math.isfinite(got), f"{kernel} {case}: {got}"
    if want == 0.0:
        print(f"FUSION-KERNELS {kernel} {case}: exactly 0 wanted, got {got}")
        assert got == 0.0
        return
    print(f"FUSION-KERNELS {kernel} {case}: rel-L2 {abs(got - want) / abs(want):.3e} max-rel {abs(got - want) / abs(want):.3e}")
    assert abs(got - want) <= LOSS_RTOL * abs(want), f"{kernel} {case}: {got} vs {want}"


# ---------------------------------------------------------------- operand builders
@pytest.mark.parametrize("case", ref.ROTCAT_CASES, ids=lambda c: "V%d_B%d_cf%d_%s_%s" % (c[0], c[1], c[2], "rel" if c[3] else "norel", c[4]))
def test_relative_rotation_and_rotcat(case):
    V, B, cf, use_rel, kind = case
    c = ref.rotcat_inputs(V, B, cf)
    D, vi, vj = c["D"], c["vi"], c["vj"]
    tag = "V%d B%d cf%d %s %s" % (V, B, cf, "rel" if use_rel else "no-rel", kind)
    rel_d = nan(D, B, 3, 3)
    ops.relative_rotation(c["rot"].to(dev()), i32(vi), i32(vj), rel_d, B, V, D)
    hold("relative_rotation", tag, rel_d, ref.relative_rotation(c["rot"], vi, vj), BUILD)
    # the builders get the float32 rel of the case table (kernel and reference read the same numbers)
    rel = c["rel"] if use_rel else None
    src_of, S = ref.src_table(V, kind)
    feat = c["lifted"] if kind == "view" else c["feats"]
    x = nan(D, B, cf + 3 * NVEC)
    ops.rotcat_fwd(c["img"].to(dev()), feat.to(dev()), rel.to(dev()) if use_rel else None, i32(vi), i32(src_of), x, B, D, cf, NVEC)
    hold("rotcat_fwd", tag, x, ref.rotcat(c["img"], feat, rel, vi, src_of), BUILD)
    assert torch.equal(x[..., :cf].cpu(), c["img"][vi]), "the image-feature columns are a copy"
    if not use_rel:
        assert torch.equal(x[..., cf:].cpu(), feat[src_of].flatten(-2, -1)), "ignore_rotmat: the feature columns are a copy"
    # backward: the kernel writes dfeat[src_of[d]] (no sum), so the table is a permutation: the partner direction, or - iteration 0 -
    # the direction itself, summed per source view by segment_sum afterwards (heads.py)
    bsrc, _ = ref.src_table(V, "partner" if kind == "partner" else "ident")
    gx = ref.randn((D, B, cf + 3 * NVEC), 20 + V)
    dfeat = nan(D, B, 3, NVEC)
    ops.rotcat_bwd(gx.to(dev()), rel.to(dev()) if use_rel else None, i32(bsrc), dfeat, B, D, cf, NVEC)
    hold("rotcat_bwd", tag, dfeat, ref.rotcat_bwd(gx, rel, bsrc, D, cf), BUILD)


@pytest.mark.parametrize("n", [1, 255, 257])
def test_rotation_matrix_2d(n):
    """R = Ry(yaw) Rx(-pitch) and its transpose past one workgroup of 256 (the golden fixture has 32 rows)."""
    hp = ref.rand((n, 2), 15) * 2 - 1
    p, y = -hp[:, 0].double(), hp[:, 1].double()
    one, zero = torch.ones_like(p), torch.zeros_like(p)
    rx = torch.stack([one, zero, zero, zero, p.cos(), -p.sin(), zero, p.sin(), p.cos()], 1).view(-1, 3, 3)
    ry = torch.stack([y.cos(), zero, y.sin(), zero, one, zero, -y.sin(), zero, y.cos()], 1).view(-1, 3, 3)
    for inverse in (False, True):
        rot = nan(n, 3, 3)
        ops.rotation_matrix_2d(hp.to(dev()), rot, inverse)
        hold("rotation_matrix_2d", "n%d inverse%d" % (n, inverse), rot, (ry @ rx).transpose(1, 2) if inverse else ry @ rx, BUILD)


@pytest.mark.parametrize("case", ref.ROTCAT_EXT_CASES, ids=lambda c: "V%d_B%d_cf%d_ld%d_apply%d_append%d" % c)
def test_rotcat_ext(case):
    V, B, cf, ld, ap, ad = case
    c = ref.rotcat_inputs(V, B, cf, seed=3)
    D, vi = c["D"], c["vi"]
    kind = "partner" if ld == 2060 else "view"
    tag = "V%d B%d cf%d ld%d apply%d append%d %s" % (V, B, cf, ld, ap, ad, kind)
    src_of, S = ref.src_table(V, kind)
    feat = c["lifted"] if kind == "view" else c["feats"]
    rel = c["rel"]
    rel_d = rel.to(dev())
    x = nan(D, B, ld)
    ops.rotcat_ext_fwd(c["img"].to(dev()), feat.to(dev()), rel_d if ap else None, rel_d if ad else None, i32(vi), i32(src_of), x, ld, B, D, cf, NVEC)
    hold("rotcat_ext_fwd", tag, x, ref.rotcat_ext(c["img"], feat, rel if ap else None, rel if ad else None, vi, src_of, ld), BUILD)
    used = cf + 3 * NVEC + (9 if ad else 0)
    assert ld > used and float(x[..., used:].abs().max()) == 0.0, "the padding columns must be exactly 0"
    if ad:
        assert torch.equal(x[..., used - 9:used].cpu(), rel.flatten(-2, -1)), "the appended rotation is a copy"
    # backward: a gradient whose appended / padding columns are NaN - the kernel must not read them
    bsrc, _ = ref.src_table(V, "partner" if kind == "partner" else "ident")
    gx = ref.randn((D, B, ld), 30 + V)
    gd = gx.clone()
    gd[..., cf + 3 * NVEC:] = float("nan")
    dfeat = nan(D, B, 3, NVEC)
    ops.rotcat_ext_bwd(gd.to(dev()), ld, rel_d if ap else None, i32(bsrc), dfeat, B, D, cf, NVEC)
    hold("rotcat_ext_bwd", tag, dfeat, ref.rotcat_ext_bwd(gx, rel if ap else None, bsrc, D, cf), BUILD)


@pytest.mark.parametrize("case", ref.IBN_CASES, ids=lambda c: "V%d_B%d_%s_%s" % (c[0], c[1], "train" if c[2] else "eval", c[3]))
def test_ibn_scales_and_paircat(case):
    V, B, training, kind = case
    c = ref.ibn_inputs(V, B, kind)
    D, vi, src_of = c["D"], c["vi"], c["src_of"]
    tag = "V%d B%d %s %s" % (V, B, "train" if training else "eval", kind)
    a_d, f_d, rel_d = c["a"].to(dev()), c["feat"].to(dev()), c["rel"].to(dev())
    rm_d = c["rm"].clone().to(dev())
    scales_d = nan(2 * D, NVEC)
    ops.ibn_scales(a_d, f_d, i32(vi), i32(src_of), rm_d, training, MOM, EPS, scales_d, B, D, NVEC)
    want_s, want_rm = ref.ibn_scales(c["a"], c["feat"], vi, src_of, c["rm"], training, MOM, EPS)
    hold("ibn_scales", tag, scales_d, want_s, ref.IBN_SCALES_BAR)
    if training:
        hold("ibn_scales.running_mean", tag, rm_d, want_rm, BUILD)
    else:
        assert torch.equal(rm_d.cpu(), c["rm"]), "eval must leave running_mean untouched"
    # paircat with the reference's scales rounded to float32 (independent of the kernel above), and as the head input
    s32 = want_s.float()
    x = nan(D, B, 6 * NVEC)
    ops.paircat_fwd(a_d, f_d, rel_d, s32.to(dev()), i32(vi), i32(src_of), x, B, D, NVEC)
    hold("paircat_fwd", tag + " scales+rel", x, ref.paircat(c["a"], c["feat"], c["rel"], s32, vi, src_of), BUILD)
    x = nan(D, B, 6 * NVEC)
    ops.paircat_fwd(a_d, f_d, None, None, i32(vi), i32(src_of), x, B, D, NVEC)
    want = ref.paircat(c["a"], c["feat"], None, None, vi, src_of)
    hold("paircat_fwd", tag + " plain", x, want, BUILD)
    assert torch.equal(x.cpu(), want.float()), "without scales and rotation the head input is a copy"
    bsrc, _ = ref.src_table(V, "partner" if kind == "partner" else "ident")
    gx = ref.randn((D, B, 6 * NVEC), 50 + V + B)
    for name, r, s in (("scales+rel", c["rel"], s32), ("plain", None, None)):
        da_dir, dfeat = nan(D, B, 3, NVEC), nan(D, B, 3, NVEC)
        ops.paircat_bwd(gx.to(dev()), r.to(dev()) if r is not None else None, s.to(dev()) if s is not None else None, i32(bsrc), da_dir, dfeat, B, D, NVEC)
        want_a, want_f = ref.paircat_bwd(gx, r, s, bsrc, D)
        hold("paircat_bwd.da", tag + " " + name, da_dir, want_a, BUILD)
        hold("paircat_bwd.dfeat", tag + " " + name, dfeat, want_f, BUILD)


@pytest.mark.parametrize("case", ref.SEGSUM_CASES, ids=lambda c: "V%d_B%d_cf%d_S%d_acc%d" % c)
def test_segment_sum(case):
    V, B, cf, segs, acc = case
    vi, _ = ref.directed_pairs(V)
    D, stride = len(vi), cf + 3 * NVEC
    x = ref.randn((D, B, stride), 60 + V)
    out0 = ref.randn((segs, B, cf), 61 + V)
    out = out0.clone().to(dev()) if acc else nan(segs, B, cf)
    ops.segment_sum(x.to(dev()), stride, cf, i32(vi), out, B, D, segs, acc)
    hold("segment_sum", "V%d B%d cf%d segments%d acc%d" % case, out, ref.segment_sum(x, cf, vi, segs, out0 if acc else None), BUILD)
    empty = out[V].cpu()                                         # no direction feeds segment V
    assert torch.equal(empty, out0[V]) if acc else float(empty.abs().max()) == 0.0


@pytest.mark.parametrize("n", ref.STREAM_NS)
def test_axpby_and_scale_by(n):
    x, y = ref.randn((n,), 70), ref.randn((n,), 71)
    xd, yd = x.to(dev()), y.clone().to(dev())
    ops.axpby(xd, yd, 1.7, -0.3)
    hold("axpby", "n%d a1.7 b-0.3" % n, yd, 1.7 * x.double() - 0.3 * y.double(), BUILD)
    yd = nan(n)
    ops.axpby(xd, yd, 0.6, 0.0)
    hold("axpby", "n%d b0 onto NaN" % n, yd, 0.6 * x.double(), BUILD)
    s = torch.tensor([0.37], dtype=torch.float32)
    out = nan(n)
    ops.scale_by(xd, s.to(dev()), out)
    hold("scale_by", "n%d" % n, out, x.double() * s.double(), BUILD)
    assert torch.equal(out.cpu(), x * s), "one float32 product per element"


# ---------------------------------------------------------------- the <= 4-wide Linear
@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("rows,k,nout", ref.SKINNY_CASES)
def test_linear_skinny(rows, k, nout, with_bias, with_mask):
    tag = "%dx%dx%d bias%d mask%d" % (rows, k, nout, with_bias, with_mask)
    x = torch.relu(ref.randn((rows, k), 80))
    w, b, dy = ref.randn((nout, k), 81) * k ** -0.5, ref.randn((nout,), 82), ref.randn((rows, nout), 83)
    xd, wd, bd, dyd = x.to(dev()), w.to(dev()), b.to(dev()) if with_bias else None, dy.to(dev())
    y = nan(rows, nout)
    ops.linear_skinny_fwd(xd, wd, bd, y, rows, k, nout)
    hold("linear_skinny_fwd", tag, y, ref.skinny_fwd(x, w, b if with_bias else None), RTOL)
    mask = x if with_mask else None
    want_dx, want_dw, want_db = ref.skinny_bwd(dy, x, w, mask)
    dx, dw, db, slot = nan(rows, k), nan(nout, k), nan(nout) if with_bias else None, torch.zeros(1, device=dev())
    ops.linear_skinny_bwd(dyd, xd, wd, xd if with_mask else None, dx, dw, db, rows, k, nout, False, slot)
    hold("linear_skinny_bwd.dx", tag, dx, want_dx, RTOL)
    hold("linear_skinny_bwd.dw", tag, dw, want_dw, RTOL)
    if with_bias:
        hold("linear_skinny_bwd.db", tag, db, want_db, RTOL)
    assert torch.equal(slot, dx.abs().max().reshape(1)), "dx_absmax must be max |dx| bit for bit"
    # accumulate onto non-zero dw / db
    dw0, db0 = ref.randn((nout, k), 84), ref.randn((nout,), 85)
    dw2, db2, dx2 = dw0.clone().to(dev()), db0.clone().to(dev()) if with_bias else None, nan(rows, k)
    ops.linear_skinny_bwd(dyd, xd, wd, xd if with_mask else None, dx2, dw2, db2, rows, k, nout, True, None)
    _, want_dw2, want_db2 = ref.skinny_bwd(dy, x, w, mask, dw0, db0)
    hold("linear_skinny_bwd.dw", tag + " accumulate", dw2, want_dw2, RTOL)
    if with_bias:
        hold("linear_skinny_bwd.db", tag + " accumulate", db2, want_db2, RTOL)
    assert torch.equal(dx2, dx), "dx does not depend on accumulate or on the abs-max slot"
    # each half alone: the same bits, and nothing else written
    dx3 = nan(rows, k)
    ops.linear_skinny_bwd(dyd, xd, wd, xd if with_mask else None, dx3, None, None, rows, k, nout, False, None)
    assert torch.equal(dx3, dx)
    dw3, db3 = nan(nout, k), nan(nout) if with_bias else None
    ops.linear_skinny_bwd(dyd, xd, wd, xd if with_mask else None, None, dw3, db3, rows, k, nout, False, None)
    assert torch.equal(dw3, dw) and (not with_bias or torch.equal(db3, db))


# ---------------------------------------------------------------- losses
@pytest.mark.parametrize("n", ref.ANGULAR_NS)
def test_gaze_angular_loss(n):
    pred, gt = ref.angular_inputs(n)
    rw = 0.37 / n
    want_th, want_loss, want_d = ref.angular_loss(pred, gt, float(np.float32(rw)))
    pd, gd = pred.to(dev()), gt.to(dev())
    loss, dpred, theta = nan(1), nan(n, 2), nan(n)
    ops.gaze_angular_loss(pd, gd, n, rw, loss, False, dpred, theta)
    hold_value("gaze_angular_loss.loss", "n%d" % n, loss, want_loss)
    hold("gaze_angular_loss.theta", "n%d" % n, theta, want_th, LOSS_RTOL)
    hold_grad("gaze_angular_loss.dpred", "n%d" % n, dpred, want_d)
    # accumulate onto a non-zero loss; no gradient / no theta wanted: the same value
    acc = torch.full((1,), 3.25, device=dev())
    ops.gaze_angular_loss(pd, gd, n, rw, acc, True, None, None)
    hold_value("gaze_angular_loss.loss", "n%d accumulate" % n, acc, 3.25 + float(want_loss))
    assert float(acc) == float(torch.tensor(3.25) + loss.cpu()[0]), "accumulate adds the same float32 value"
    alone = nan(1)
    ops.gaze_angular_loss(pd, gd, n, rw, alone, False, None, None)
    assert torch.equal(alone, loss)


def test_gaze_angular_loss_coincident_rows_are_finite():
    """pred == gt bit for bit: sim is 1 up to a few ulp, so acos gives at most sqrt(2 * 4 * 2^-24) = 7e-4 rad = 0.04 degree, and the
    gradient is either 0 (sim clamped) or finite - never NaN or inf."""
    n = 257
    _, gt = ref.angular_inputs(n, 9)
    gd = gt.to(dev())
    loss, dpred, theta = nan(1), nan(n, 2), nan(n)
    ops.gaze_angular_loss(gd.clone(), gd, n, 1.0 / n, loss, False, dpred, theta)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dpred).all()) and bool(torch.isfinite(theta).all())
    print(f"FUSION-KERNELS gaze_angular_loss.coincident n{n}: max theta {float(theta.max()):.3e} deg, max |dpred| {float(dpred.abs().max()):.3e}")
    assert float(theta.max()) <= 0.1 and float(theta.min()) >= 0.0 and abs(float(loss)) <= 0.1
    multi_loss, multi_d = nan(1), nan(1, n, 2)
    ops.gaze_angular_loss_multi(gd.clone().view(1, n, 2), gd, 1, 1, n, [1.0], multi_loss, multi_d)
    assert bool(torch.isfinite(multi_loss).all()) and bool(torch.isfinite(multi_d).all()) and abs(float(multi_loss)) <= 0.1


@pytest.mark.parametrize("iters,dirs,batch", ref.ANGULAR_MULTI_CASES)
def test_gaze_angular_loss_multi(iters, dirs, batch):
    tag = "I%d D%d B%d" % (iters, dirs, batch)
    n = dirs * batch
    pred, gt = ref.angular_multi_inputs(iters, dirs, batch)
    w = [float(np.float32(0.01 + 1e-4 * i)) for i in range(iters * dirs)]         # distinct per (iteration, direction)
    want_loss, want_d = ref.angular_loss_multi(pred, gt, w, dirs, batch)
    pd, gd = pred.to(dev()), gt.to(dev())
    loss, dpred = nan(1), nan(iters, n, 2)
    ops.gaze_angular_loss_multi(pd, gd, iters, dirs, batch, w, loss, dpred)
    hold_value("gaze_angular_loss_multi.loss", tag, loss, want_loss)
    hold_grad("gaze_angular_loss_multi.dpred", tag, dpred, want_d)
    alone = nan(1)
    ops.gaze_angular_loss_multi(pd, gd, iters, dirs, batch, w, alone, None)
    assert torch.equal(alone, loss)
    # ... and against iters x dirs single launches that accumulate (w * (1 / B) and w / B may round differently: 1e-6, not bits)
    acc, d1 = torch.zeros(1, device=dev()), nan(iters, n, 2)
    for it in range(iters):
        for d in range(dirs):
            rows = slice(d * batch, (d + 1) * batch)
            ops.gaze_angular_loss(pd[it, rows].contiguous(), gd[rows].contiguous(), batch, w[it * dirs + d] / batch, acc, True, d1[it, rows], None)
    hold("gaze_angular_loss_multi.loss", tag + " vs single launches", loss, acc, 1e-6)
    hold("gaze_angular_loss_multi.dpred", tag + " vs single launches", dpred, d1, 1e-6)


@pytest.mark.parametrize("n", ref.LP_NS)
@pytest.mark.parametrize("p", [1, 2])
def test_gaze_lp_loss(p, n):
    pred = ref.randn((n,), 90)
    label = pred + 0.3 * ref.randn((n,), 91)
    label[2::5] = pred[2::5]
    want_loss, want_d = ref.lp_loss(pred, label, p)
    loss, dpred = nan(1), nan(n)
    ops.gaze_lp_loss(pred.to(dev()), label.to(dev()), n, p, loss, dpred)
    hold_value("gaze_lp_loss.loss", "p%d n%d" % (p, n), loss, want_loss)
    hold_grad("gaze_lp_loss.dpred", "p%d n%d" % (p, n), dpred, want_d)
    if n > 2:
        assert float(dpred[2::5].abs().max()) == 0.0, "pred == label: the gradient is exactly 0"
    alone = nan(1)
    ops.gaze_lp_loss(pred.to(dev()), label.to(dev()), n, p, alone, None)
    assert torch.equal(alone, loss)


# ---------------------------------------------------------------- pools / layout
@pytest.mark.parametrize("n,h,w,c", ref.MAXPOOL_CASES)
def test_maxpool_against_aten_ties_included(n, h, w, c):
    tag = "%dx%dx%dx%d" % (n, h, w, c)
    x = ref.maxpool_input(n, h, w, c)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    gy = ref.randn((n, c, ho, wo), 95)
    want_y, want_code, want_dx = ref.maxpool(x, gy)
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev())
    y, am = nan(n, ho, wo, c), nan(n, ho, wo, c, dtype=torch.uint8)
    ops.maxpool_fwd(xd, y, am, n, h, w, c, ho, wo)
    hold("maxpool_fwd", tag, y, want_y, BUILD)
    assert torch.equal(y.cpu(), want_y), "y must equal ATen's bit for bit"
    wrong = int((am.cpu() != want_code).sum())
    print(f"FUSION-KERNELS maxpool_fwd.argmax {tag}: {wrong} of {am.numel()} differ from ATen's (ties in {ref.maxpool_tie_fraction(x):.2f} of the windows)")
    assert wrong == 0, "argmax must be ATen's winner (the first maximum in scan order) at every element"
    dx = nan(n, h, w, c)
    ops.maxpool_bwd(gy.permute(0, 2, 3, 1).contiguous().to(dev()), am, dx, n, h, w, c, ho, wo)
    hold("maxpool_bwd", tag, dx, want_dx, BUILD)


@pytest.mark.parametrize("n,hw,c", ref.AVGPOOL_CASES)
def test_avgpool(n, hw, c):
    tag = "%dx%dx%d" % (n, hw, c)
    x, gy = ref.randn((n, hw, c), 96), ref.randn((n, c), 97)
    y = nan(n, c)
    ops.avgpool_fwd(x.to(dev()), y, n, hw, c)
    hold("avgpool_fwd", tag, y, ref.avgpool(x), BUILD)
    dx = nan(n, hw, c)
    ops.avgpool_bwd(gy.to(dev()), dx, n, hw, c)
    hold("avgpool_bwd", tag, dx, ref.avgpool_bwd(gy, hw), BUILD)


def test_layout_round_trip_odd_sizes():
    n, c, h, w = 2, 3, 5, 7
    img = ref.randn((n, c, h, w), 98)
    d4 = nan(n, h, w, 4)
    ops.nchw_to_nhwc4(img.to(dev()), d4, n, c, h, w)
    assert torch.equal(d4[..., :3].cpu(), img.permute(0, 2, 3, 1)) and float(d4[..., 3].abs().max()) == 0.0
    back = nan(n, c, h, w)
    ops.nhwc4_to_nchw(d4, back, n, c, h, w)
    assert torch.equal(back.cpu(), img)
    print("FUSION-KERNELS nchw_to_nhwc4/nhwc4_to_nchw 2x3x5x7: rel-L2 0.000e+00 max-rel 0.000e+00")


# ---------------------------------------------------------------- head level: the variants on the materialised fp32 path, V > 2
def rel_l2(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float((got - want).norm()) / (float(want.norm()) + 1e-300)


HEAD_VARIANTS = {"encode_rotmat": {"encode_rotmat": True}, "share_feature": {"share_feature": True},
                 "share_weights_encode_rotmat": {"share_weights": True, "encode_rotmat": True}}


@pytest.mark.parametrize("V,B", [(3, 5), (4, 3)])
@pytest.mark.parametrize("name", list(HEAD_VARIANTS))
def test_head_variants_beyond_two_views_against_the_fp64_oracle(name, V, B):
    """head.forward (eval and training) / head.backward of the variants whose fusers take the materialised operands (rotcat_ext,
    ibn_scales + paircat) at D = 6 and 12 directions against the float64 loop of R.fuse_pair over R.view_pairs(V) on ONE shared state
    dict (the IntensityBatchNorm buffers walk on from pair to pair), with the HIP forward's ReLU patterns imposed."""
    from oracle import restatement as R
    from rot_mvgaze_amd import synth
    from rot_mvgaze_amd.arch import Variant
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    from rot_mvgaze_amd.model import MultiViewGaze
    depth, I = 18, 3
    v = Variant(**HEAD_VARIANTS[name])
    torch.set_num_threads(min(16, __import__("os").cpu_count() or 1))
    sd = {k: np.array(x) for k, x in synth.make_state_dict(depth, 0, I, True, variant=v).items()}
    m = MultiViewGaze(depth, I, v)
    m.load_state_dict({k: torch.from_numpy(x) for k, x in sd.items()}, strict=True)
    m.to(dev()).train()
    m.ensure_layout()
    torch.manual_seed(7)
    cf = m._fc_dim
    img_feat = (torch.rand(V, B, cf, device=dev()) * 2.0).contiguous()
    rot = rotation_matrix_2d(torch.rand(B * V, 2, device=dev()) - 0.5).reshape(B, V, 3, 3)
    head = m._head
    head.split, head.mixed = True, False                       # (as the model sets them for fp32: these variants never take the split path)
    D = V * (V - 1)
    f64 = [img_feat[i].double().cpu().requires_grad_(True) for i in range(V)]
    r64 = rot.double().cpu()
    rm_keys = [k for k in sd if k.endswith("_batchnorm.running_mean")]
    assert (len(rm_keys) == I) == v.share_feature

    def oracle(tape, training):
        sd64 = {k: torch.from_numpy(x).double() for k, x in sd.items() if x.dtype == np.float32 and not k.startswith("_feat_extractor")}
        for k, t in sd64.items():
            if k not in rm_keys:
                t.requires_grad_(True)
        hl_mask = (tape["hl"][0] > 0).cpu().view(V, B, -1)
        lift64 = [R.lift(sd64, f64[i], hl_mask[i]) for i in range(V)]
        fu = head.fusers[0]
        outs = []
        for p, (i, j) in enumerate(R.view_pairs(V)):
            masks = {}
            for it in range(I):
                _, Hf, _, Hh, _ = tape["saved"][it]
                hf = [(h > 0).cpu().view(D, B, -1)[..., :fu.fout[l]] for l, h in enumerate(Hf)]      # (hidden widths are zero-padded to 4)
                hh = (Hh[0] > 0).cpu().view(D, B, -1)
                masks[("fuse", it)] = [[h[2 * p + s] for h in hf] for s in (0, 1)]
                masks[("head", it)] = [hh[2 * p], hh[2 * p + 1]]
            outs.append(R.fuse_pair(sd64, I, f64[i], f64[j], lift64[i], lift64[j], r64[:, i], r64[:, j], masks, v, training))
        return sd64, outs

    def compare(feats, preds, outs, what):
        worst = 0.0
        for p, o in enumerate(outs):
            for it in range(I):
                for s in (0, 1):
                    d = 2 * p + s
                    ef = rel_l2(feats[it, d].reshape(B, -1), o[f"iter_{it}"][f"feat_{s}"].reshape(B, -1))
                    ep = rel_l2(preds[it, d], o[f"iter_{it}"][f"pred_gaze_{s}"])
                    worst = max(worst, ef, ep)
                    assert ef < 2e-5 and ep < 2e-5, (what, it, d, ef, ep)
        print(f"FUSION-KERNELS head.{name} V{V} B{B} {what}: rel-L2 {worst:.3e} max-rel {worst:.3e}")

    # eval forward: the buffers are read, not moved
    ibn = head.ibn if v.share_feature else []
    before = [b.clone() for b in ibn]
    _, feats, preds, tape = head.forward(img_feat, rot, True, False)
    assert tape["mode"] == "fp32" and bool(torch.isfinite(feats).all()) and bool(torch.isfinite(preds).all())
    assert all(torch.equal(a, b) for a, b in zip(before, ibn))
    feats_eval, preds_eval = feats.clone(), preds.clone()
    if v.share_feature:                                         # the only variant whose forward depends on the mode
        compare(feats, preds, oracle(tape, False)[1], "eval forward")
    # training forward and backward
    _, feats, preds, tape = head.forward(img_feat, rot, True, True)
    assert tape["mode"] == "fp32"
    if not v.share_feature:                                     # same launches, deterministic kernels: the oracle comparison below holds for both
        assert torch.equal(feats_eval, feats) and torch.equal(preds_eval, preds)
        print(f"FUSION-KERNELS head.{name} V{V} B{B} eval forward: bit-equal to the training forward")
    gpred = torch.randn_like(preds)
    m._sink.active = False
    m._sink.begin()
    dimg = head.backward(tape, None, None, gpred, m._sink, None)
    m._sink.active = False
    torch.cuda.synchronize()
    sd64, outs = oracle(tape, True)
    compare(feats, preds, outs, "training forward")
    for it, k in enumerate(sorted(rm_keys)):
        l2, mx, _, _ = measure(f"head.{name}.running_mean", "V%d B%d it%d" % (V, B, it), ibn[it].reshape(-1), sd64[k].reshape(-1))
        assert mx <= 1e-6, (k, mx)
    total = 0.0
    for p, o in enumerate(outs):
        for it in range(I):
            for s in (0, 1):
                total = total + (o[f"iter_{it}"][f"pred_gaze_{s}"] * gpred[it, 2 * p + s].double().cpu()).sum()
    total.backward()
    worst = 0.0
    for i in range(V):
        e = rel_l2(dimg[i], f64[i].grad)
        worst = max(worst, e)
        assert e < 2e-5, ("image-feature gradient", i, e)
    groups = {}
    for k, prm in m.named_parameters(remove_duplicate=False):
        if not k.startswith("_feat_extractor"):
            groups.setdefault(id(prm), (prm, []))[1].append(k)
    checked = 0
    for prm, names in groups.values():
        refs = [sd64[k].grad for k in names if sd64[k].grad is not None]
        if not refs:
            continue
        e = rel_l2(m._grad_views[id(prm)], sum(refs))
        worst = max(worst, e)
        checked += 1
        assert e < 2e-5, (names, e)
    assert checked == 4 + (1 if v.share_weights else I) * (2 * head.fusers[0].n + 4)
    print(f"FUSION-KERNELS head.{name} V{V} B{B} gradients ({checked} parameters): rel-L2 {worst:.3e} max-rel {worst:.3e}")
