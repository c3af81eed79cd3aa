"""Every launch form of the split conv kernels (csrc/conv_split.hip) at kernel level, on small shapes.

Which instantiation a shape runs is decided on the host: split_plan() picks the K loop of igemm_split16_kernel (single-stage /
two-stage pipeline) from the tile count, the K-steps and the CUs the planners may use, wgrad_split_tile() picks one of seven
tiles and the pixel addressing of wgrad_split_kernel.  The shape lists of test_split_gpu.py leave forms unrun on a 256-CU
device - above all igemm_split16_kernel<128, *> with one stage and the DMA loader, which does almost all conv work of the bench
default.  Here ops.set_reserved_cus() moves the plan instead of the shape: with all but 8 CUs reserved the pipeline is chosen
only up to 16 tiles (32 with >= 48 K-steps), so a shape of a few dozen tiles runs single-stage, and with none reserved it runs
pipelined.  Every forward / backward-data case runs under both settings and FIRST asserts, through the host-only plan queries
(mvg_conv_fprop_split_stages, mvg_conv_dgrad_split_stages, mvg_conv_wgrad_split_tile: answered by the code the launches plan
with), that it ran the form it is here for: a later change of the plan that moves a shape to another form fails the guard
instead of silently losing the coverage.

Bars: test_split_gpu.py's, imported - relative L2 against the float64 F.conv2d / autograd reference <= SPLIT_VS_F64 (2e-6) and
<= SPLIT_VS_FP32_KERNEL (3) x the fp32-MFMA kernel's error on the same inputs + 1e-7; the fused reduce against the two-launch
sequence as test_split_dgrad_fused_with_bn_backward_reduce has it (dx, mx bit for bit; sums to 2e-5 sqrt(rows)).  Across the two
settings forward and backward-data results are torch.equal - a condition, not a tolerance: both K loops multiply the same
fragments in ascending K-step order and share one epilogue.  (Backward-weight is not compared across settings: the slab count
changes the summation order.)

Measured on an MI355X (profiles/r10_split_forms_errors.txt), relative L2 against float64, smallest .. largest over the cases
(the bars above are test_split_gpu.py's and were not refitted to these); every comparison prints its figure before it asserts:
  forward          pipelined 8.6e-08 .. 5.2e-07   single-stage the same bits   (fp32-MFMA kernel 7.5e-08 .. 5.9e-07)
  ... affine       pipelined 8.9e-08 .. 4.7e-07   single-stage the same bits   (fp32-MFMA kernel 6.9e-08 .. 5.3e-07)
  backward-data    pipelined 4.8e-08 .. 4.5e-07   single-stage the same bits   (fp32-MFMA kernel 5.4e-08 .. 7.2e-07)
  backward-weight  every CU  7.1e-08 .. 2.4e-07   8 CUs 7.1e-08 .. 3.5e-07     (fp32-MFMA kernel 3.5e-08 .. 2.5e-07; at most 2.1 x it)
"""
import contextlib
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from test_split_gpu import SPLIT_VS_F64, SPLIT_VS_FP32_KERNEL, dev, rel_l2

pytestmark = pytest.mark.gpu

NAN = float("nan")


@contextlib.contextmanager
def reserved_cus(n):
    from rot_mvgaze_amd import ops
    try:
        ops.set_reserved_cus(n)
        yield
    finally:
        ops.set_reserved_cus(0)


def settings():
    """(name, CUs to reserve, K-loop stages the forward / backward-data cases must get): every CU, and 8 CUs."""
    from rot_mvgaze_amd._lib import lib
    cus = lib().mvg_device_cus()
    assert cus >= 64, "the form guards are written for a device with many more than 8 CUs"
    return (("all CUs", 0, 2), ("8 CUs", cus - 8, 1))


def case_id(c):
    return "g%d_n%d_h%dx%d_%dto%d_k%d_s%d" % c[:8]


def sq(G, N, h, cin, cout, k, stride, pad):
    return (G, N, h, h, cin, cout, k, stride, pad)


def desc(case):
    from rot_mvgaze_amd._lib import ConvDesc
    G, N, h, w_, cin, cout, k, st, pad = case
    return ConvDesc(G, N, h, w_, cin, cout, k, k, st, pad, (h + 2 * pad - k) // st + 1, (w_ + 2 * pad - k) // st + 1)


class Problem:
    """Inputs of one conv as test_split_conv_fprop_dgrad_wgrad makes them (a gradient-sized dy with its scale; the addend
    gradient-sized too, so that the bars weigh dx itself), their sp copies and the float64 F.conv2d / autograd reference: y,
    dx + addend, dw."""

    def __init__(self, case):
        from rot_mvgaze_amd import ops
        G, N, h, w_, cin, cout, k, st, pad = case
        torch.manual_seed(sum(case))
        self.d = d = desc(case)
        self.x = torch.relu(torch.randn(G, N, h, w_, cin, device=dev()))
        self.w = torch.randn(cout, k, k, cin, device=dev()) * (1.0 / (k * k * cin) ** 0.5)
        gy = torch.randn(G, N, d.ho, d.wo, cout, device=dev())
        self.add = torch.randn_like(self.x) * 2.0 ** -20      # of dx's own size: next to an O(1) addend dx would be rounding noise
        self.xs, self.gys = ops.split_f32(self.x), ops.split_f32(gy * 2.0 ** -20, 2.0 ** 28)
        self.gy = gy * 2.0 ** -20
        self.wk, self.wt = ops.split_weights(d, self.w, True)
        xr = self.x.double().view(G * N, h, w_, cin).permute(0, 3, 1, 2).requires_grad_(True)
        wr = self.w.double().permute(0, 3, 1, 2).requires_grad_(True)
        yr = F.conv2d(xr, wr, None, st, pad)
        yr.backward(self.gy.double().view(G * N, d.ho, d.wo, cout).permute(0, 3, 1, 2))
        self.y_ref = yr.detach().permute(0, 2, 3, 1).reshape(G, N, d.ho, d.wo, cout)
        self.dx_ref = xr.grad.permute(0, 2, 3, 1).reshape(self.x.shape) + self.add.double()
        self.dw_ref = wr.grad.permute(0, 2, 3, 1)


def within_bars(name, e_split, e_fp32):
    print(f"FORMS {name}: split {e_split:.3e} fp32-MFMA {e_fp32:.3e}")
    assert e_split <= SPLIT_VS_F64 and e_split <= SPLIT_VS_FP32_KERNEL * e_fp32 + 1e-7, \
        f"{name}: split {e_split:.2e}, fp32-MFMA kernel {e_fp32:.2e}"


# G, N, h, cin, cout, k, stride, pad; tiles and K-steps of the 128-column plan (tiles = groups x row tiles x column tiles)
FPROP_CASES = [
    (1, 2, 56, 64, 256, 1, 1, 0),       # 98 tiles, 2 K-steps
    (1, 10, 15, 32, 128, 1, 1, 0),      # 18 tiles, ONE K-step: the pipelined kernel runs only its prologue; ragged last row tile
    (1, 10, 15, 96, 160, 1, 1, 0),      # 3 K-steps, ragged second column tile
    (2, 6, 14, 256, 256, 3, 1, 1),      # 40 tiles, 72 K-steps, tap-major K order
    (3, 7, 7, 512, 2048, 1, 1, 0),      # 16 column tiles
]
DGRAD_CASES = [
    (1, 10, 15, 128, 32, 1, 1, 0),      # 18 tiles, one K-step
    (2, 6, 14, 256, 256, 3, 1, 1),      # 40 tiles, 72 K-steps, tap-major K order
    (3, 7, 7, 512, 2048, 1, 1, 0),      # 36 tiles, 64 K-steps
    (2, 3, 27, 128, 128, 3, 2, 1),      # four ragged parity classes, 38 tiles, one single-tap class
]
# the fused BatchNorm-backward reduce: the stride-1 3x3 case and both stride-2 cases; the 1x1 one keeps three classes without
# taps (40 tiles, 30 of them epilogue only; WITHOUT the reduce it is 10 tiles and pipelined under both settings)
BNREDUCE_CASES = [(2, 6, 14, 256, 256, 3, 1, 1), (2, 3, 27, 128, 128, 3, 2, 1), (2, 3, 28, 128, 256, 1, 2, 0)]
AFFINE_CASES = [(1, 2, 56, 64, 256, 1, 1, 0), (2, 6, 14, 256, 256, 3, 1, 1)]


def ids8(cases):
    return [case_id(sq(*c)) for c in cases]


@pytest.mark.parametrize("case", FPROP_CASES, ids=ids8(FPROP_CASES))
def test_split_fprop_single_stage_and_pipelined(case):
    """mvg_conv_fprop_split, y and the BatchNorm statistics partials, under both K loops: each against float64, then bit for bit
    against each other."""
    from rot_mvgaze_amd import ops
    pb = Problem(sq(*case))
    d, G, cout = pb.d, pb.d.groups, pb.d.cout
    rows = d.n * d.ho * d.wo
    y32 = torch.full(pb.y_ref.shape, NAN, device=dev())
    ops.conv_fprop(d, pb.x, pb.w, y32, None, False, None)
    e32 = rel_l2(y32, pb.y_ref)
    P, rpp = ops.conv_stats_partials_split(d)
    covered = (rows + rpp - 1) // rpp                 # (the last tile's second partial may lie beyond the rows: never written)
    got = {}
    for name, res, stages in settings():
        with reserved_cus(res):
            assert ops.conv_fprop_split_stages(d) == stages, f"{name}: this shape no longer runs the {stages}-stage K loop"
            y = torch.full(pb.y_ref.shape, NAN, device=dev())
            stats = torch.full((G, P, 2, cout), NAN, device=dev())
            ops.conv_fprop_split(d, pb.xs, pb.wk, y, stats)
        within_bars(f"fprop {stages}-stage {case_id(sq(*case))}", rel_l2(y, pb.y_ref), e32)
        # the statistics partials describe the rows they cover: sums, and squares centred on the partial's own mean
        yg = y.view(G, rows, cout).double()
        for p in range(covered):
            blk = yg[:, p * rpp:min((p + 1) * rpp, rows)]
            torch.testing.assert_close(stats[:, p, 0].double(), blk.sum(1), rtol=1e-4, atol=1e-4 * float(blk.abs().sum(1).max()))
            q = ((blk - blk.mean(1, keepdim=True)) ** 2).sum(1)
            torch.testing.assert_close(stats[:, p, 1].double(), q, rtol=1e-3, atol=1e-5 * float(q.max()) + 1e-12)
        got[stages] = (y, stats[:, :covered].clone())
    assert torch.equal(got[1][0], got[2][0]), "y: the single-stage and the pipelined K loop differ"
    assert torch.equal(got[1][1], got[2][1]), "statistics partials: the single-stage and the pipelined K loop differ"


@pytest.mark.parametrize("case", DGRAD_CASES, ids=ids8(DGRAD_CASES))
def test_split_dgrad_single_stage_and_pipelined(case):
    """mvg_conv_dgrad_split with an addend, and with the addend aliasing dx, under both K loops."""
    from rot_mvgaze_amd import ops
    pb = Problem(sq(*case))
    d = pb.d
    dx32 = torch.empty_like(pb.x)
    ops.conv_dgrad(d, pb.gy, pb.w, dx32, None, pb.add)
    e32 = rel_l2(dx32, pb.dx_ref)
    got = {}
    for name, res, stages in settings():
        with reserved_cus(res):
            assert ops.conv_dgrad_split_stages(d) == stages, f"{name}: this shape no longer runs the {stages}-stage K loop"
            dx = torch.full(pb.x.shape, NAN, device=dev())
            ops.conv_dgrad_split(d, pb.gys, pb.wt, dx, pb.add)
            dx_in_place = pb.add.clone()
            ops.conv_dgrad_split(d, pb.gys, pb.wt, dx_in_place, dx_in_place)
        within_bars(f"dgrad {stages}-stage {case_id(sq(*case))}", rel_l2(dx, pb.dx_ref), e32)
        within_bars(f"dgrad-in-place {stages}-stage {case_id(sq(*case))}", rel_l2(dx_in_place, pb.dx_ref), e32)
        got[stages] = (dx, dx_in_place)
    assert torch.equal(got[1][0], got[2][0]), "dx: the single-stage and the pipelined K loop differ"
    assert torch.equal(got[1][1], got[2][1]), "dx (addend in place): the single-stage and the pipelined K loop differ"


@pytest.mark.parametrize("case", BNREDUCE_CASES, ids=ids8(BNREDUCE_CASES))
@pytest.mark.parametrize("mask", ["bits", "affine"])
def test_split_dgrad_bnreduce_single_stage_and_pipelined(case, mask):
    """mvg_conv_dgrad_split_bnreduce (gamma and the dy-scale slot given) == mvg_conv_dgrad_split + the reduce pass, as
    test_split_dgrad_fused_with_bn_backward_reduce compares them, under both K loops; then everything the fused launch and its
    finalize leave is the same bits under both."""
    from rot_mvgaze_amd import ops
    G, N, h, cin, cout, k, st, pad = case
    torch.manual_seed(sum(case) + len(mask))
    d = desc(sq(*case))
    rows = N * h * h
    w = torch.randn(cout, k, k, cin, device=dev()) * (1.0 / (k * k * cout) ** 0.5)
    gy = torch.randn(G, N, d.ho, d.wo, cout, device=dev())
    add = torch.randn(G, N, h, h, cin, device=dev())
    _, wt = ops.split_weights(d, w, True)
    gys = ops.split_f32(gy)
    y = torch.randn(G, rows, cin, device=dev()) * 1.5 + 0.3
    mean, invstd = torch.randn(G, cin, device=dev()) * 0.1 + 0.3, torch.rand(G, cin, device=dev()) + 0.4
    scale, shift = torch.rand(G, cin, device=dev()) + 0.5, torch.randn(G, cin, device=dev()) * 0.3
    gamma = torch.rand(cin, device=dev()) + 0.5
    bits = torch.randint(0, 16, (G * rows * cin // 4,), dtype=torch.uint8, device=dev()) if mask == "bits" else None
    ra = (scale, shift) if mask == "affine" else None
    got = {}
    for name, res, stages in settings():
        with reserved_cus(res):
            assert ops.conv_dgrad_split_stages(d, True) == stages, f"{name}: this shape no longer runs the {stages}-stage K loop"
            # reference: two launches
            dx_ref = torch.full((G, N, h, h, cin), NAN, device=dev())
            ops.conv_dgrad_split(d, gys, wt, dx_ref, add)
            s_ref = [torch.full((G, cin), NAN, device=dev()) for _ in range(2)]
            dg_ref, db_ref = torch.full((cin,), 0.5, device=dev()), torch.full((cin,), -0.25, device=dev())
            g2 = dx_ref.view(G, rows, cin)
            am_ref = torch.full((G, cin), NAN, device=dev())
            ops.bn_bwd_reduce_split(g2, bits, y, mean, invstd, G, rows, cin, s_ref[0], s_ref[1], dg_ref, db_ref, True, am_ref, ra, dz_out=g2)
            # fused
            dx = torch.full_like(dx_ref, NAN)
            s = [torch.full((G, cin), NAN, device=dev()) for _ in range(2)]
            dg, db = torch.full((cin,), 0.5, device=dev()), torch.full((cin,), -0.25, device=dev())
            am = torch.full((G, cin), NAN, device=dev())
            sinv = torch.full((1,), NAN, device=dev())
            ops.conv_dgrad_split_bnreduce(d, gys, wt, dx, add, y, bits, mean, invstd, ra, s[0], s[1], dg, db, True, am, gamma, sinv)
        assert torch.equal(dx, dx_ref), f"{name}: masked gradient"
        assert torch.equal(am, am_ref) and torch.equal(am, dx.view(G, rows, cin).abs().amax(dim=1)), f"{name}: max |masked gradient|"
        for a, want, what in ((s[0], s_ref[0], "s1"), (s[1], s_ref[1], "s2"), (dg, dg_ref, "dgamma"), (db, db_ref, "dbeta")):
            err = (a - want).abs().max().item()
            assert err <= 2e-5 * max(want.abs().max().item(), 1.0) * (rows ** 0.5), f"{name}: {what}: {err:.3e}"
        assert bool(torch.isfinite(sinv).all())
        got[stages] = (dx, am, s[0], s[1], dg, db, sinv)
    for a, b, what in zip(got[1], got[2], ("dx", "mx", "s1", "s2", "dgamma", "dbeta", "dy's 2^-k")):
        assert torch.equal(a, b), f"{what}: the single-stage and the pipelined K loop differ"


@pytest.mark.parametrize("case", AFFINE_CASES, ids=ids8(AFFINE_CASES))
@pytest.mark.parametrize("res,relu,out_sp", [("sp", True, True), (None, False, False)], ids=["residual_sp_relu_out_sp", "plain"])
def test_split_fprop_affine_single_stage_and_pipelined(case, res, relu, out_sp):
    """mvg_conv_fprop_split_affine (the affine epilogue: residual in sp + ReLU + sp output, and the plain form) against float64 as
    test_split_inference_forward_with_folded_batchnorm has it, under both K loops."""
    from rot_mvgaze_amd import ops
    G, N, h, cin, cout, k, st, pad = case
    torch.manual_seed(sum(case))
    d = desc(sq(*case))
    x = torch.relu(torch.randn(G, N, h, h, cin, device=dev()))
    w = torch.randn(cout, k, k, cin, device=dev()) * (1.0 / (k * k * cin) ** 0.5)
    scale, shift = torch.rand(cout, device=dev()) + 0.5, torch.randn(cout, device=dev()) * 0.3
    r = torch.randn(G, N, d.ho, d.wo, cout, device=dev()) if res else None
    ref = F.conv2d(x.double().view(G * N, h, h, cin).permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), None, st, pad).permute(0, 2, 3, 1)
    ref = ref.reshape(G, N, d.ho, d.wo, cout) * scale.double() + shift.double()
    if res:
        ref = ref + r.double()
    if relu:
        ref = torch.relu(ref)
    want = torch.empty(G, N, d.ho, d.wo, cout, device=dev())
    ops.conv_fprop_affine(d, x, w, want, scale, shift, r, relu)
    e32 = rel_l2(want, ref)
    assert e32 <= SPLIT_VS_F64, f"fp32-MFMA kernel (the yardstick of the bars below) {e32:.2e} against float64"
    wk, _ = ops.split_weights(d, w, False)
    xs, rs = ops.split_f32(x), ops.split_f32(r) if res else None
    got = {}
    for name, rsv, stages in settings():
        with reserved_cus(rsv):
            assert ops.conv_fprop_split_stages(d) == stages, f"{name}: this shape no longer runs the {stages}-stage K loop"
            out = ops.sp_empty(G, N, d.ho, d.wo, cout, device=dev()) if out_sp else torch.empty_like(want)
            out.fill_(NAN)
            ops.conv_fprop_split_affine(d, xs, wk, out, scale, shift, rs, relu)
        within_bars(f"fprop-affine {stages}-stage {case_id(sq(*case))}", rel_l2(ops.merge_sp(out) if out_sp else out, ref), e32)
        got[stages] = out
    assert torch.equal(got[1], got[2]), "affine output: the single-stage and the pipelined K loop differ"


# ---- backward-weight: seven tiles (cout rows x r*s*cin columns), each with and without incremental pixel addressing
# (ho * wo >= 32).  G, N, h, w, cin, cout, k, stride, pad
WGRAD_CASES = [
    (2, 16, 6, 6, 128, 256, 1, 1, 0),   # 128 x 128 (cin = 128 1x1: not a multiple of 192 or 256 columns), several slabs
    (1, 2, 5, 5, 160, 128, 1, 1, 0),    # 128 x 128, ragged second column tile, ho * wo = 25
    (1, 22, 5, 6, 128, 128, 1, 1, 0),   # 128 x 128 at ho * wo = 30: just below the incremental form's threshold
    (2, 3, 8, 8, 64, 64, 1, 1, 0),      # 64 x 64
    (1, 4, 2, 2, 32, 32, 1, 1, 0),      # 64 x 64, half-empty tile both ways, ho * wo = 4
    (1, 2, 6, 6, 256, 128, 1, 1, 0),    # 128 x 256 at ho * wo = 36: just past the threshold
    (2, 2, 5, 5, 256, 128, 1, 1, 0),    # 128 x 256, ho * wo = 25
    (1, 16, 8, 8, 256, 256, 3, 1, 1),   # 128 x 256, 18 tiles: four slabs on every CU, ONE on 8 CUs
    (1, 2, 6, 6, 64, 128, 3, 1, 1),     # 128 x 192
    (1, 3, 5, 5, 128, 128, 3, 1, 1),    # 128 x 192, ho * wo = 25
    (1, 2, 9, 9, 64, 128, 3, 2, 1),     # 128 x 192, stride 2, ho * wo = 25
    (1, 16, 8, 8, 128, 256, 3, 1, 1),   # 128 x 192, 12 tiles: four slabs / two
    (1, 40, 6, 6, 96, 128, 1, 1, 0),    # 128 x 64, ragged second column tile
    (1, 4, 2, 2, 64, 128, 1, 1, 0),     # 128 x 64, ho * wo = 4
    (1, 2, 6, 6, 64, 64, 3, 1, 1),      # 64 x 192
    (1, 2, 5, 5, 64, 64, 3, 1, 1),      # 64 x 192, ho * wo = 25
    (2, 8, 12, 12, 128, 64, 1, 1, 0),   # 64 x 128
    (1, 2, 2, 2, 32, 64, 3, 1, 1),      # 64 x 128, ho * wo = 4
    (1, 7, 1, 1, 128, 64, 1, 1, 0),     # 64 x 128, ho * wo = 1: 7 pixels in a 16-pixel K-step
]
WGRAD_FORMS = [(128, 128, True), (128, 128, False), (128, 128, False), (64, 64, True), (64, 64, False), (128, 256, True),
               (128, 256, False), (128, 256, True), (128, 192, True), (128, 192, False), (128, 192, False), (128, 192, True),
               (128, 64, True), (128, 64, False), (64, 192, True), (64, 192, False), (64, 128, True), (64, 128, False), (64, 128, False)]
WGRAD_SCALED_X = {WGRAD_CASES[0], WGRAD_CASES[9]}         # ... also through _xs with a scaled x operand
WGRAD_SLABS_DIFFER = {WGRAD_CASES[7], WGRAD_CASES[11]}     # the two settings must sum different slab counts


@pytest.mark.parametrize("case,form", list(zip(WGRAD_CASES, WGRAD_FORMS)), ids=[case_id(c) for c in WGRAD_CASES])
def test_split_wgrad_every_tile_form(case, form):
    """mvg_conv_wgrad_split (plain, accumulate, a scaled x operand) on the tile form the case is here for, summed over the slab
    counts of both settings."""
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import lib
    pb = Problem(case)
    d = pb.d
    assert ops.conv_wgrad_split_tile(d) == form, "this shape no longer runs the tile form it is here for"
    dw32 = torch.empty_like(pb.w)
    ops.conv_wgrad(d, pb.x, pb.gy, dw32)
    e32 = rel_l2(dw32, pb.dw_ref)
    slabs = []
    for name, res, _ in settings():
        with reserved_cus(res):
            slabs.append(lib().mvg_conv_wgrad_splits_split(C.byref(d)))
            dw = torch.full(pb.w.shape, NAN, device=dev())
            ops.conv_wgrad_split(d, pb.xs, pb.gys, dw)
            dw_acc = torch.ones_like(pb.w)
            ops.conv_wgrad_split(d, pb.xs, pb.gys, dw_acc, True)
            dw_xs = None
            if case in WGRAD_SCALED_X:
                dw_xs = torch.full(pb.w.shape, NAN, device=dev())
                ops.conv_wgrad_split(d, ops.split_f32(pb.x, 2.0 ** 6), pb.gys, dw_xs)
        what = "wgrad %dx%d%s %s, %d slabs, %s" % (form[0], form[1], " incr" if form[2] else "", name, slabs[-1], case_id(case))
        within_bars(what, rel_l2(dw, pb.dw_ref), e32)
        assert rel_l2(dw_acc, pb.dw_ref + 1.0) <= SPLIT_VS_F64, what + ": accumulate"
        if dw_xs is not None:
            within_bars(what + " (scaled x)", rel_l2(dw_xs, pb.dw_ref), e32)
    if case in WGRAD_SLABS_DIFFER:
        assert slabs[0] > slabs[1], f"slab counts {slabs}: the two settings no longer sum this shape differently"


def test_split_wgrad_cases_cover_every_tile_form():
    """The plan's answers over WGRAD_CASES are all seven tiles times both pixel addressings: no form is left unrun."""
    from rot_mvgaze_amd import ops
    seen = {ops.conv_wgrad_split_tile(desc(c)) for c in WGRAD_CASES}
    tiles = ((128, 256), (128, 192), (128, 128), (128, 64), (64, 192), (64, 128), (64, 64))
    assert seen == {(bm, bn, incr) for bm, bn in tiles for incr in (True, False)}
