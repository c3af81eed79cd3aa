"""mvg_conv_fprop_split_bnapply (csrc/conv_split.hip, the block-output-forming loader): the BatchNorm apply pass of a residual
block's last unit formed inside the forward launch of the next block's conv1.  The reference is the two-launch form it
replaces - ops.bn_apply_split, then ops.conv_fprop_split on that output - and the bar is equality, bit for bit: the loader
evaluates bn_apply_sp_kernel's expressions in its order (an explicit fma, the add, the ReLU, the mask bit from the unscaled
value, then the power-of-two scale), splits with the same helper and feeds the matrix cores the same fragments in the same K
order; tiling and epilogue are the plain launch's, so the BatchNorm statistics partials are compared with torch.equal too."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (G, N, h, cin, cout): 75 rows - one ragged tile, two groups; 162 rows - a full tile and a ragged one, 16 K-steps, 128
# columns; two K-steps, three groups; 13 tiles
SHAPES = [(2, 3, 5, 256, 64), (1, 2, 9, 512, 128), (3, 2, 14, 64, 64), (1, 2, 28, 256, 128), (1, 1, 3, 32, 64)]
SENTINEL = 1234.0


def dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("sinvs", [(1.0, 1.0), (2.0 ** -4, 2.0 ** 3)], ids=["unit_scales", "out2e-4_res2e3"])
@pytest.mark.parametrize("form", ["identity", "affine"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda c: "g%d_n%d_h%d_%dto%d" % c)
def test_fprop_forms_its_input_in_its_loader(shape, form, sinvs):
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import ConvDesc
    G, N, h, cin, cout = shape
    out_sinv, res_sinv = sinvs
    torch.manual_seed(sum(shape) + len(form))
    d = ConvDesc.make(G, N, h, h, cin, cout, 1, 1, 0)
    rows = N * h * h
    w = torch.randn(cout, 1, 1, cin, device=dev()) * (1.0 / cin ** 0.5)
    wk, _ = ops.split_weights(d, w, False)
    # the producer: conv output, (scale, shift) of both signs of the result - about half the values negative before the ReLU
    y = torch.randn(G, rows, cin, device=dev()) * 1.5
    scale, shift = torch.rand(G, cin, device=dev()) + 0.5, torch.randn(G, cin, device=dev()) * 0.3
    res = torch.randn(G, rows, cin, device=dev()) * 1.2
    dead = cin // 2 + 3                      # pre-ReLU value exactly 0: the bit must be 0
    scale[:, dead] = 0.0
    shift[:, dead] = 0.0
    res[:, :, dead] = 0.0
    if form == "identity":
        residual = ops.split_f32(res, 1.0 / res_sinv)       # stored times 2^k, read back times 2^-k
        assert (residual.sinv is None) == (res_sinv == 1.0)
        ra = None
    else:
        residual = res
        ra = (torch.rand(G, cin, device=dev()) + 0.5, torch.randn(G, cin, device=dev()) * 0.3)
        ra[0][:, dead] = 0.0
        ra[1][:, dead] = 0.0
    osv = None if out_sinv == 1.0 else torch.full((1,), out_sinv, device=dev())
    P, _ = ops.conv_stats_partials_split(d)

    # reference: the apply pass, then the plain forward
    out_ref = ops.sp_empty(G, N, h, h, cin, device=dev())
    out_ref.sinv = osv
    bits_ref = ops.bn_apply_split(y, scale, shift, residual, True, out_ref, G, rows, cin, ra, want_bits=True)
    y2_ref = torch.full((G, N, h, h, cout), SENTINEL, device=dev())
    st_ref = torch.full((G, P, 2, cout), SENTINEL, device=dev())
    ops.conv_fprop_split(d, out_ref, wk, y2_ref, st_ref)
    pre = ops.merge_sp(out_ref)
    frac = float((pre == 0).float().mean())
    assert 0.3 < frac < 0.7, frac                           # the ReLU cut about half
    assert not bool(bits_ref.view(G, rows, cin // 4)[:, :, dead // 4].bitwise_and(1 << (dead % 4)).any())

    # merged: out and the bits are outputs; they sit in front of guard rows that must stay untouched
    buf = ops.sp_empty(G * rows + 8, cin, device=dev()).fill_(SENTINEL)
    out = buf[:G * rows].view(G, N, h, h, cin // 8, 2, 8)
    out.sinv = osv
    nb = G * rows * cin // 4
    bbuf = torch.full((nb + 64,), 0xA5, dtype=torch.uint8, device=dev())
    y2 = torch.full((G, N, h, h, cout), SENTINEL, device=dev())
    st = torch.full((G, P, 2, cout), SENTINEL, device=dev())
    y_before, res_before = y.clone(), residual.clone()
    ops.conv_fprop_split_bnapply(d, out, y, scale, shift, residual, wk, y2, st, ra, bbuf[:nb])
    assert torch.equal(out, out_ref), "sp out (both pieces)"
    assert bool((buf[G * rows:] == SENTINEL).all()), "rows behind out were written"
    assert torch.equal(bbuf[:nb], bits_ref), "ReLU mask bits"
    assert bool((bbuf[nb:] == 0xA5).all()), "bytes behind the mask bits were written"
    assert torch.equal(y, y_before) and torch.equal(residual, res_before), "y and the residual are inputs"
    assert torch.equal(y2, y2_ref), "the consumer's conv output"
    assert torch.equal(st, st_ref), "BatchNorm statistics partials"
    # without the bits (a forward that keeps no tape)
    out3 = ops.sp_empty(G, N, h, h, cin, device=dev()).fill_(SENTINEL)
    out3.sinv = osv
    y3 = torch.full((G, N, h, h, cout), SENTINEL, device=dev())
    ops.conv_fprop_split_bnapply(d, out3, y, scale, shift, residual, wk, y3, None, ra, None)
    assert torch.equal(out3, out_ref) and torch.equal(y3, y2_ref)


@pytest.mark.parametrize("bad,msg", [(dict(st=2), "1x1, stride 1, pad 0 only"), (dict(k=3, pad=1), "1x1, stride 1, pad 0 only"),
                                     (dict(cout=256), "cout must be 64 or 128"), (dict(cin=48), "cin must be a multiple of 32"),
                                     (dict(cin=1024), "at most 512"), (dict(sp_with_affine=True), "the residual is an sp identity")],
                         ids=["stride2", "3x3", "cout256", "cin48", "cin1024", "sp_with_affine"])
def test_entry_rejects_what_the_loader_does_not_cover(bad, msg):
    """The C entry's own argument checks: the usual error return and message, nothing launched."""
    import ctypes as C
    from rot_mvgaze_amd._lib import ConvDesc, lib
    G, N, h = 1, 2, 8
    cin, cout = bad.get("cin", 64), bad.get("cout", 64)
    k, st, pad = bad.get("k", 1), bad.get("st", 1), bad.get("pad", 0)
    d = ConvDesc.make(G, N, h, h, cin, cout, k, st, pad)
    keep = []

    def z(*shape):
        keep.append(torch.zeros(*shape, device=dev()))
        return keep[-1].data_ptr()
    big = G * N * h * h * max(cin, cout) * k * k
    aff = z(G, cin) if bad.get("sp_with_affine") else None
    rc = lib().mvg_conv_fprop_split_bnapply(C.byref(d), z(big), None, z(big), z(G, cin), z(G, cin), z(big), 1, aff, aff, None, None,
                                            z(big), None, z(big), None, None)
    assert rc != 0
    err = lib().mvg_last_error().decode()
    assert "fprop_split_bnapply" in err and msg in err, err
    torch.cuda.synchronize()


def test_switch_off_is_the_two_launch_sequence_and_on_changes_no_bit():
    """Backbone.fuse_bn_apply_fprop on / off over a ResNet-50 training step at V = 2, B = 2, 64 x 64: loss, every parameter
    gradient and the running statistics bit-equal.  At this batch the launch plan pipelines the 128-column consumers (at
    most two tiles per CU), so the two 64-column pairs of layer1 merge - one with the affine residual, one with the sp identity."""
    import numpy as np
    from rot_mvgaze_amd import ops, synth
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    from rot_mvgaze_amd.losses import IterationLoss, StereoL1Loss
    from rot_mvgaze_amd.model import FeatRotationSymm
    B, hw = 2, 64
    sd = synth.make_state_dict(50, 0, 3, perturb_bn=True)
    inp = synth.make_inputs(B, 2, 1234, hw)
    img, hp, gt = (torch.from_numpy(inp[k]) for k in ("img", "head_pose", "gt_gaze"))
    metrics = IterationLoss(StereoL1Loss(rel_weight=0.01, reference_decay=1.0), iter_decay=0.5)
    results, calls = {}, {}
    real = ops.conv_fprop_split_bnapply
    for fuse in (False, True):
        model = FeatRotationSymm(backbone_depth=50, num_iter=3)
        model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
        model.to(dev()).train()
        model._ensure_layout(dev())
        assert model._backbone.fuse_bn_apply_fprop is True
        model._backbone.fuse_bn_apply_fprop = fuse
        forms = []

        def counted(d, out_sp, bn_y, scale, shift, residual, *a, **kw):
            forms.append("identity" if ops.is_sp(residual) else "affine")
            return real(d, out_sp, bn_y, scale, shift, residual, *a, **kw)
        ops.conv_fprop_split_bnapply = counted
        try:
            data = {"img_0": img[:, 0].contiguous().to(dev()), "img_1": img[:, 1].contiguous().to(dev()),
                    "rot_0": rotation_matrix_2d(hp[:, 0].contiguous().to(dev())),
                    "rot_1": rotation_matrix_2d(hp[:, 1].contiguous().to(dev())),
                    "gt_gaze": gt[:, 0].contiguous().to(dev()), "gt_gaze_1": gt[:, 1].contiguous().to(dev())}
            loss = metrics(model(data))
            loss.backward()
            torch.cuda.synchronize()
        finally:
            ops.conv_fprop_split_bnapply = real
        calls[fuse] = forms
        results[fuse] = (loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None},
                         {k: b.clone() for k, b in model.named_buffers() if "running" in k})
    assert calls[False] == [] and calls[True] == ["affine", "identity"], calls
    assert torch.equal(results[True][0], results[False][0])
    assert results[True][1].keys() == results[False][1].keys() and len(results[True][1]) > 100
    for k, gfalse in results[False][1].items():
        assert torch.equal(results[True][1][k], gfalse), k
    assert results[True][2].keys() == results[False][2].keys() and len(results[True][2]) > 100
    for k, bfalse in results[False][2].items():
        assert torch.equal(results[True][2][k], bfalse), k
