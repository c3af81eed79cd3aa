"""mvg_conv_dgrad_split_bnapply_bnreduce (csrc/conv_split.hip, the dy-forming loader): the BatchNorm-backward apply pass
of a 1x1 stride-1 unit formed inside that unit's backward-data launch.  The reference is the two-launch form it replaces -
ops.bn_bwd_apply_split on (dz, y, ..., dy_sinv), then ops.conv_dgrad_split_bnreduce on that dy - and the bar is equality,
bit for bit: the loader evaluates the same bn_dy expression, splits with the same helper and feeds the matrix cores the same
fragments in the same K order; the launch keeps the two-launch form's tiling (128-row tiles, one column tile), so the fused
reduce's partials - s1 / s2 / dgamma / dbeta / max |dx| - are added in the same order too and are compared with torch.equal,
not to a summation-order bound."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (G, N, h, cin, cout): 75 rows - one ragged tile; 162 rows - a full tile and a ragged one; two K-steps; five K-steps with
# cout not a multiple of 64; 49 tiles
SHAPES = [(2, 3, 5, 64, 256), (1, 2, 9, 128, 512), (3, 2, 14, 64, 64), (2, 5, 9, 128, 160), (1, 2, 56, 64, 256), (1, 1, 3, 64, 32)]
SENTINEL = 1234.0


def dev():
    return torch.device("cuda:0")


def _unit_inputs(G, rows, cout, mag):
    """The unit's own BatchNorm-backward state: a masked gradient dz of magnitude mag (about half of it zeros, like a ReLU's),
    y, statistics, gamma, one dead channel (huge invstd, no gradient), and the sums / bound / 2^-k a reduce pass leaves."""
    from rot_mvgaze_amd import ops
    dz = torch.randn(G, rows, cout, device=dev()) * mag * (torch.rand(G, rows, cout, device=dev()) > 0.5)
    y = torch.randn(G, rows, cout, device=dev()) * 1.5 + 0.3
    mean, invstd = torch.randn(G, cout, device=dev()) * 0.1 + 0.3, torch.rand(G, cout, device=dev()) + 0.4
    gamma = torch.rand(cout, device=dev()) + 0.5
    dead = cout // 2 + 3
    dz[:, :, dead] = 0.0
    invstd[:, dead] = 1e4
    # (sums in torch: the stand-alone reduce pass does not take every channel count used here; they are inputs to both forms alike)
    s1, s2 = dz.sum(dim=1), (dz * (y - mean[:, None]) * invstd[:, None]).sum(dim=1)
    mx = dz.abs().amax(dim=1)
    scratch = ops.sp_empty(G, rows, cout, device=dev())
    ops.bn_bwd_apply_split(dz, y, mean, invstd, gamma, s1, s2, G, rows, cout, scratch, None, mx)     # computes the 2^-k from the bound
    sinv = scratch.sinv
    return dz, y, mean, invstd, gamma, s1, s2, mx, sinv


@pytest.mark.parametrize("mag", [1.0, 2.0 ** -20, 2.0 ** 10], ids=["mag1", "mag2e-20", "mag2e10"])
@pytest.mark.parametrize("mask", ["bits", "affine", "none"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda c: "g%d_n%d_h%d_%dfrom%d" % c)
def test_dgrad_forms_dy_in_its_loader(shape, mask, mag):
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import ConvDesc
    G, N, h, cin, cout = shape
    torch.manual_seed(sum(shape) + len(mask))
    d = ConvDesc.make(G, N, h, h, cin, cout, 1, 1, 0)
    rows = N * h * h
    w = torch.randn(cout, 1, 1, cin, device=dev()) * (1.0 / cout ** 0.5)
    _, wt = ops.split_weights(d, w, True)
    add = torch.randn(G, N, h, h, cin, device=dev()) * mag
    dz, y, mean, invstd, gamma, us1, us2, umx, sinv = _unit_inputs(G, rows, cout, mag)
    if mag != 1.0:
        assert float(sinv) != 1.0
    # the unit that receives dx: its conv output, statistics, ReLU mask in one of the three forms, gamma
    by = torch.randn(G, rows, cin, device=dev()) * 1.5 + 0.3
    bmean, binvstd = torch.randn(G, cin, device=dev()) * 0.1 + 0.3, torch.rand(G, cin, device=dev()) + 0.4
    scale, shift = torch.rand(G, cin, device=dev()) + 0.5, torch.randn(G, cin, device=dev()) * 0.3
    bits = torch.randint(0, 16, (G * rows * cin // 4,), dtype=torch.uint8, device=dev()) if mask == "bits" else None
    ra = (scale, shift) if mask == "affine" else None
    bgamma = torch.rand(cin, device=dev()) + 0.5

    def outputs():
        return dict(dx=torch.full((G, N, h, h, cin), float("nan"), device=dev()), s1=torch.empty(G, cin, device=dev()),
                    s2=torch.empty(G, cin, device=dev()), dg=torch.full((cin,), 0.5, device=dev()),
                    db=torch.full((cin,), -0.25, device=dev()), mx=torch.full((G, cin), float("nan"), device=dev()),
                    sinv=torch.full((1,), float("nan"), device=dev()))

    # reference: the apply pass, then backward-data with the fused reduce (accumulating into dgamma / dbeta)
    dy_ref = ops.sp_empty(G, rows, cout, device=dev())
    ops.bn_bwd_apply_split(dz, y, mean, invstd, gamma, us1, us2, G, rows, cout, dy_ref, None, umx, sinv)
    r = outputs()
    ops.conv_dgrad_split_bnreduce(d, dy_ref, wt, r["dx"], add, by, bits, bmean, binvstd, ra, r["s1"], r["s2"], r["dg"], r["db"], True,
                                  r["mx"], bgamma, r["sinv"])
    # merged: dy is an output; it sits in front of guard rows that must stay untouched
    buf = ops.sp_empty(G * rows + 8, cout, device=dev()).fill_(SENTINEL)
    dy = buf[:G * rows].view(G, rows, cout // 8, 2, 8)
    dz_before = dz.clone()
    m = outputs()
    ops.conv_dgrad_split_bnapply_bnreduce(d, dy, sinv, dz, y, mean, invstd, gamma, us1, us2, rows, wt, m["dx"], add, by, bits, bmean,
                                          binvstd, ra, m["s1"], m["s2"], m["dg"], m["db"], True, m["mx"], bgamma, m["sinv"])
    assert dy.sinv is sinv
    assert torch.equal(dy, dy_ref), "sp dy (both pieces)"
    assert bool((buf[G * rows:] == SENTINEL).all()), "rows behind dy were written"
    assert torch.equal(dz, dz_before), "dz is an input"
    assert not bool(torch.isnan(m["dx"]).any())
    assert torch.equal(m["dx"], r["dx"]), "masked dx"
    assert torch.equal(m["mx"], r["mx"]), "max |dx| per (group, channel)"
    # same tiling as the two-launch form (128-row tiles, one column tile): the same partials, added in the same order
    for k in ("s1", "s2", "dg", "db", "sinv"):
        assert torch.equal(m[k], r[k]), k
    # without accumulation, the addend aliasing the result
    r2, m2 = outputs(), outputs()
    r2["dx"].copy_(add)
    m2["dx"].copy_(add)
    ops.conv_dgrad_split_bnreduce(d, dy_ref, wt, r2["dx"], r2["dx"], by, bits, bmean, binvstd, ra, r2["s1"], r2["s2"], r2["dg"], r2["db"],
                                  False, r2["mx"], bgamma, r2["sinv"])
    dy2 = ops.sp_empty(G, rows, cout, device=dev()).fill_(SENTINEL)
    ops.conv_dgrad_split_bnapply_bnreduce(d, dy2, sinv, dz, y, mean, invstd, gamma, us1, us2, rows, wt, m2["dx"], m2["dx"], by, bits,
                                          bmean, binvstd, ra, m2["s1"], m2["s2"], m2["dg"], m2["db"], False, m2["mx"], bgamma, m2["sinv"])
    assert torch.equal(dy2, dy_ref) and torch.equal(m2["dx"], r2["dx"]) and torch.equal(m2["dx"], r["dx"])
    for k in ("s1", "s2", "dg", "db", "mx", "sinv"):
        assert torch.equal(m2[k], r2[k]), k + " (no accumulation)"
    assert not torch.equal(m2["dg"], m["dg"])


@pytest.mark.parametrize("bad,msg", [(dict(st=2), "1x1, stride 1, pad 0 only"), (dict(k=3, pad=1), "1x1, stride 1, pad 0 only"),
                                     (dict(cin=256), "cin must be 64 or 128"), (dict(cout=48), "cout must be a multiple of 32"),
                                     (dict(no_scale=True), "dy_sinv")],
                         ids=["stride2", "3x3", "cin256", "cout48", "no_scale"])
def test_entry_rejects_what_the_loader_does_not_cover(bad, msg):
    """The C entry's own argument checks (called directly: the Python wrapper sizes the partials first, which has checks of
    its own): the usual error return and message, nothing launched."""
    import ctypes as C
    from rot_mvgaze_amd._lib import ConvDesc, lib
    G, N, h = 1, 2, 8
    cin, cout = bad.get("cin", 64), bad.get("cout", 64)
    k, st, pad = bad.get("k", 1), bad.get("st", 1), bad.get("pad", 0)
    d = ConvDesc.make(G, N, h, h, cin, cout, k, st, pad)
    rows = N * d.ho * d.wo
    keep = []

    def z(*shape):
        keep.append(torch.zeros(*shape, device=dev()))
        return keep[-1].data_ptr()
    big = G * N * h * h * max(cin, cout) * k * k
    sinv = None if bad.get("no_scale") else z(1)
    rc = lib().mvg_conv_dgrad_split_bnapply_bnreduce(C.byref(d), z(big), sinv, z(big), z(big), z(G, cout), z(G, cout), z(cout), z(G, cout),
                                                     z(G, cout), rows, z(big), None, z(big), None, z(big), None, z(G, cin), z(G, cin),
                                                     None, None, z(4 * big), z(G, cin), z(G, cin), None, None, 0, z(G, cin), None, None,
                                                     None)
    assert rc != 0
    err = lib().mvg_last_error().decode()
    assert "dgrad_split_bnapply_bnreduce" in err and msg in err, err
    torch.cuda.synchronize()


def test_switch_off_is_the_two_launch_sequence_and_on_changes_no_bit():
    """Backbone.fuse_bn_apply_dgrad on / off over a ResNet-50 training step: seven merged launches, every parameter gradient
    and the loss bit-equal."""
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
    real = ops.conv_dgrad_split_bnapply_bnreduce
    for fuse in (False, True):
        model = FeatRotationSymm(backbone_depth=50, num_iter=3)
        model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
        model.to(dev()).train()
        model._ensure_layout(dev())
        assert model._backbone.fuse_bn_apply_dgrad is True
        model._backbone.fuse_bn_apply_dgrad = fuse
        n = [0]

        def counted(*a, **kw):
            n[0] += 1
            return real(*a, **kw)
        ops.conv_dgrad_split_bnapply_bnreduce = counted
        try:
            data = {"img_0": img[:, 0].contiguous().to(dev()), "img_1": img[:, 1].contiguous().to(dev()),
                    "rot_0": rotation_matrix_2d(hp[:, 0].contiguous().to(dev())),
                    "rot_1": rotation_matrix_2d(hp[:, 1].contiguous().to(dev())),
                    "gt_gaze": gt[:, 0].contiguous().to(dev()), "gt_gaze_1": gt[:, 1].contiguous().to(dev())}
            loss = metrics(model(data))
            loss.backward()
            torch.cuda.synchronize()
        finally:
            ops.conv_dgrad_split_bnapply_bnreduce = real
        calls[fuse] = n[0]
        results[fuse] = (loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
    assert calls[False] == 0 and calls[True] == 7, calls
    assert torch.equal(results[True][0], results[False][0])
    assert results[True][1].keys() == results[False][1].keys() and len(results[True][1]) > 100
    for k, gfalse in results[False][1].items():
        assert torch.equal(results[True][1][k], gfalse), k
