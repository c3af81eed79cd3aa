"""mvg_augment_u8hwc_bf16 - the training augmentation stored straight as the bf16 stem's operand (NHWC8 and / or the folded
row windows) - against the chain it replaces (augment -> fp32 NHWC4 -> NCHW -> stem_rowwindow_bf16 / nchw_to_nhwc8_bf16,
same draws), against the NumPy restatement, and through the bf16 model's raw-input training path.  Every comparison is
exact, on the bf16 bits: the bf16 value is the fp32 destination's value rounded once.  Every destination is a slice in the
middle of a buffer of 0xFF bytes: the margins must keep them (no store outside) and no element may keep the 0xFFFF
pattern (every byte written; 0xFFFF is a NaN no pixel rounds to)."""
import random

import numpy as np
import pytest
import torch

import augment_bf16_ref as W
import augment_ref as R
import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd import ops, synth
from rot_mvgaze_amd.augment import RandomMultiErasing, TrainAugment
from rot_mvgaze_amd.backbone import IMAGE_MEAN, IMAGE_STD

pytestmark = pytest.mark.gpu

MARGIN = 4096                   # bf16 elements on each side of a destination (a multiple of 8: the slice stays 16-byte aligned)
SHAPES = [(3, 5, 4),            # one window per row: both pads in the same window
          (2, 3, 8),            # two windows per row
          (2, 37, 44),          # h*w not a multiple of 1024
          (2, 64, 64),          # h*w exactly one 4096-pixel pass
          (2, 72, 68)]          # a second pass with a tail


def dev():
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int16)


class Guarded:
    """A bf16 destination of `shape` in the middle of a buffer prefilled with 0xFF bytes."""

    def __init__(self, *shape):
        numel = int(np.prod(shape))
        self.buf = torch.full((numel + 2 * MARGIN,), -1, dtype=torch.int16, device=dev())
        self.dst = self.buf[MARGIN:MARGIN + numel].view(torch.bfloat16).view(*shape)
        assert self.dst.is_contiguous() and self.dst.data_ptr() % 16 == 0

    def margins_intact(self):
        return bool((self.buf[:MARGIN] == -1).all() and (self.buf[-MARGIN:] == -1).all())

    def fully_written(self):
        return not bool((self.buf[MARGIN:-MARGIN] == -1).any())

    def untouched(self):
        return bool((self.buf == -1).all())


def keep_mask(g, mask, h, w):
    """multi_erase_kernel's index rule in float32: cell = min(int(floor(i * (g / size))), g - 1) per axis."""
    if g == 0:
        return np.ones((h, w), np.float32)
    my = np.minimum(np.floor(np.arange(h, dtype=np.float32) * (np.float32(g) / np.float32(h))).astype(np.int64), g - 1)
    mx = np.minimum(np.floor(np.arange(w, dtype=np.float32) * (np.float32(g) / np.float32(w))).astype(np.int64), g - 1)
    return mask.numpy().astype(np.float32)[my][:, mx]


def restated_bf16_bits(u8, draws, bgr):
    """tests/augment_ref.py per image, ToTensor and Normalize in float32 on the CPU, times the keep-mask, rounded with
    Tensor.to(torch.bfloat16): int16 [n, h, w, 3]."""
    n, h, w, _ = u8.shape
    mean, std = torch.tensor(IMAGE_MEAN), torch.tensor(IMAGE_STD)
    out = []
    for i in range(n):
        r = draws.recs[i]
        rgb = R.augment(u8[i], r["factor"], r["order"], (r["a0"], r["cx"], r["a4"], r["cy"]), bgr)
        x = (torch.from_numpy(rgb).float().div(255) - mean) / std
        if draws.erase is not None:
            x = x * torch.from_numpy(keep_mask(draws.erase[i][0], draws.erase[i][1], h, w))[..., None]
        out.append(x.to(torch.bfloat16))
    return torch.stack(out).view(torch.int16).numpy()


@pytest.mark.parametrize("erase", [False, True], ids=["plain", "erase"])
@pytest.mark.parametrize("bgr", [False, True], ids=["rgb", "bgr"])
@pytest.mark.parametrize("n,h,w", SHAPES)
def test_both_destinations_equal_the_chain_and_the_restatement(n, h, w, bgr, erase):
    seed = 1000 * h + 10 * w + 2 * int(bgr) + int(erase) + 4       # (seeds at which every case draws a fill and a dropped cell)
    torch.manual_seed(seed), random.seed(seed), np.random.seed(seed)
    aug = TrainAugment(translate=(0.2, 0.2), scale=(0.8, 1.25),
                       erase=RandomMultiErasing([0.3, 0.6], 1.0, [0.1, 0.34]) if erase else None)
    host = np.random.RandomState(seed).randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    u8 = torch.from_numpy(host).to(dev())
    draws = aug.draw(n, h, w)
    assert not erase or all(g >= 2 for g, _ in draws.erase)
    # the parent's chain with the same draws
    nchw = aug.apply(u8, draws, out="nchw", bgr=bgr)
    rw_chain = torch.empty(n, h, w // 4, 64, dtype=torch.bfloat16, device=dev())
    ops.stem_rowwindow_bf16(nchw, rw_chain)
    n8_chain = torch.empty(n, h, w, 8, dtype=torch.bfloat16, device=dev())
    ops.nchw_to_nhwc8_bf16(nchw, n8_chain, n, 3, h, w)
    # each destination alone, then both from one launch
    rw, n8, rw2, n82 = Guarded(n, h, w // 4, 64), Guarded(n, h, w, 8), Guarded(n, h, w // 4, 64), Guarded(n, h, w, 8)
    aug.launch(u8, draws, None, None, bgr, dst_rw=rw.dst)
    aug.launch(u8, draws, None, None, bgr, dst_nhwc8=n8.dst)
    aug.launch(u8, draws, None, None, bgr, dst_nhwc8=n82.dst, dst_rw=rw2.dst)
    torch.cuda.synchronize()
    for name, g in (("rw", rw), ("nhwc8", n8), ("rw of both", rw2), ("nhwc8 of both", n82)):
        assert g.margins_intact(), f"{name}: a store outside the destination"                  # (a)
        assert g.fully_written(), f"{name}: an element of the destination was not written"     # (b)
    assert torch.equal(bits(rw.dst), bits(rw_chain))                                           # (c)
    assert torch.equal(bits(n8.dst), bits(n8_chain))                                           # (d)
    want = restated_bf16_bits(host, draws, bgr)                                                # (e)
    assert np.array_equal(bits(rw.dst).cpu().numpy(), W.row_windows(want))
    assert np.array_equal(bits(n8.dst).cpu().numpy(), W.nhwc8(want))
    assert torch.equal(bits(rw2.dst), bits(rw.dst)) and torch.equal(bits(n82.dst), bits(n8.dst))      # (f)
    # apply's two outputs are these launches
    assert torch.equal(bits(aug.apply(u8, draws, out="rw_bf16", bgr=bgr)), bits(rw.dst))
    got8 = aug.apply(u8, draws, out="nhwc8_bf16", bgr=bgr)
    assert got8.dtype == torch.bfloat16 and got8.shape == (n, h, w, 8) and torch.equal(bits(got8), bits(n8.dst))
    # the draws did something: filled pixels exist, and with the erase some cell is dropped
    filled = [(R.axis_table(w, r["a0"], r["cx"]) < 0).any() or (R.axis_table(h, r["a4"], r["cy"]) < 0).any() for r in draws.recs]
    assert any(filled)
    assert not erase or any((m == 0).any() for _, m in draws.erase)


@pytest.mark.parametrize("n,h,w", [(2, 9, 7), (1, 70, 61), (2, 5, 6)])
def test_nhwc8_alone_takes_any_width(n, h, w):
    """The NHWC8 destination has no width rule: odd widths, and 4270 pixels (a second pass with a tail)."""
    torch.manual_seed(w), random.seed(w), np.random.seed(w)
    aug = TrainAugment(translate=(0.2, 0.2), scale=(0.8, 1.25), erase=RandomMultiErasing([0.3, 0.6], 1.0, [0.1, 0.34]))
    u8 = torch.from_numpy(np.random.RandomState(w).randint(0, 256, (n, h, w, 3)).astype(np.uint8)).to(dev())
    draws = aug.draw(n, h, w)
    nchw = aug.apply(u8, draws, out="nchw", bgr=True)
    chain = torch.empty(n, h, w, 8, dtype=torch.bfloat16, device=dev())
    ops.nchw_to_nhwc8_bf16(nchw, chain, n, 3, h, w)
    g = Guarded(n, h, w, 8)
    aug.launch(u8, draws, None, None, True, dst_nhwc8=g.dst)
    torch.cuda.synchronize()
    assert g.margins_intact() and g.fully_written()
    assert torch.equal(bits(g.dst), bits(chain))


@pytest.mark.parametrize("bgr", [False, True])
def test_identity_augment_equals_the_bf16_preprocess(bgr):
    n, h, w = 3, 40, 44
    aug = TrainAugment(brightness=0, contrast=0, saturation=0, scale=None, translate=None)
    u8 = torch.from_numpy(np.random.RandomState(4).randint(0, 256, (n, h, w, 3)).astype(np.uint8)).to(dev())
    want = torch.empty(n, h, w, 8, dtype=torch.bfloat16, device=dev())
    ops.preprocess_u8hwc_resize_bf16(u8, want, n, h, w, h, w, IMAGE_MEAN, IMAGE_STD, bgr)
    assert torch.equal(bits(aug(u8, out="nhwc8_bf16", bgr=bgr)), bits(want))
    rw = torch.empty(n, h, w // 4, 64, dtype=torch.bfloat16, device=dev())
    ops.stem_rowwindow_bf16(want[..., :3].float().permute(0, 3, 1, 2).contiguous(), rw)       # bf16 -> fp32 -> bf16 is exact
    assert torch.equal(bits(aug(u8, out="rw_bf16", bgr=bgr)), bits(rw))


def test_bad_arguments_raise_and_queue_nothing():
    n, h, w = 2, 8, 8
    src = torch.zeros(n, h, w, 3, dtype=torch.uint8, device=dev())
    aug = TrainAugment()
    recs = aug.draw(n, h, w).recs
    rdev = torch.from_numpy(recs.view(np.uint8).reshape(-1)).to(dev())
    g8, grw = Guarded(n, h, w, 8), Guarded(n, h, w // 4, 64)

    def call(**kw):
        a = dict(src=src, recs=rdev, dst_nhwc8=g8.dst, dst_rw=grw.dst, masks=None, grid=None, gmax=0, n=n, h=h, w=w, mean=IMAGE_MEAN,
                 std=IMAGE_STD, swap_rb=False, recs_host=recs)
        a.update(kw)
        ops.augment_u8hwc_bf16(**a)
    with pytest.raises(RuntimeError, match="no destination"):
        call(dst_nhwc8=None, dst_rw=None)
    src6 = torch.zeros(n, h, 6, 3, dtype=torch.uint8, device=dev())
    g6 = Guarded(n, h, 1, 64)                                       # (6 // 4 windows: the size ops expects; the library refuses w)
    with pytest.raises(RuntimeError, match=r"dst_rw.*w % 4 == 0 \(w = 6\)"):
        call(src=src6, w=6, dst_nhwc8=None, dst_rw=g6.dst)
    grid = torch.zeros(n, dtype=torch.int32, device=dev())
    masks = torch.zeros(n, 4, dtype=torch.float32, device=dev())
    with pytest.raises(RuntimeError, match="come together"):
        call(masks=masks, gmax=2)
    with pytest.raises(RuntimeError, match="come together"):
        call(grid=grid)
    bad = recs.copy()
    bad["order"][1] = (0, 0, 2)
    with pytest.raises(RuntimeError, match="record 1.*not a permutation"):
        call(recs_host=bad)
    with pytest.raises(RuntimeError, match="std must be positive"):
        call(std=(0.2, 0.0, 0.2))
    # TrainAugment's own refusals
    with pytest.raises(ValueError, match="multiple of 4"):
        aug.apply(src6, aug.draw(n, h, 6), out="rw_bf16")
    with pytest.raises(ValueError, match="multiple of 4"):
        aug.launch(src6, aug.draw(n, h, 6), None, None, dst_rw=g6.dst)
    with pytest.raises(ValueError, match="a launch each"):
        aug.launch(src, aug.draw(n, h, w), None, torch.empty(n, h, w, 4, device=dev()), dst_nhwc8=g8.dst)
    torch.cuda.synchronize()
    assert g8.untouched() and grw.untouched() and g6.untouched()
    call()                                                          # ... and the same arguments, left alone, launch
    torch.cuda.synchronize()
    assert g8.margins_intact() and g8.fully_written() and grw.margins_intact() and grw.fully_written()


@pytest.mark.parametrize("B,hw,stem_rw", [(2, 64, True),            # B ho (wo / 2) = 1024: the row-window stem
                                          (3, 40, False)])          # 600, not a multiple of 64: the NHWC8 stem
def test_bf16_model_trains_from_raw_patches(B, hw, stem_rw):
    """ResNet-18, V=2, compute_dtype = bfloat16, train mode, BGR uint8 patches: a step with model.input_augment equals a step
    of the same weights fed TrainAugment.apply(out="nchw") with the same draws (reseeded: view order, then image order) -
    outputs, loss, every gradient and every buffer, bit for bit."""
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    from rot_mvgaze_amd.losses import IterationLoss, StereoL1Loss
    from rot_mvgaze_amd.model import FeatRotationSymm
    rng = np.random.RandomState(9)
    u8 = [torch.from_numpy(rng.randint(0, 256, (B, hw, hw, 3)).astype(np.uint8)).to(dev()) for _ in range(2)]
    inp = synth.make_inputs(B, 2, 1234, hw)
    hp, gt = (torch.from_numpy(inp[k]).to(dev()) for k in ("head_pose", "gt_gaze"))
    rest = {"rot_0": rotation_matrix_2d(hp[:, 0].contiguous()), "rot_1": rotation_matrix_2d(hp[:, 1].contiguous()),
            "gt_gaze": gt[:, 0].contiguous(), "gt_gaze_1": gt[:, 1].contiguous()}
    sd = {k: torch.from_numpy(np.array(v)) for k, v in synth.make_state_dict(18, 0, 3, perturb_bn=True).items()}
    metrics = IterationLoss(StereoL1Loss(rel_weight=0.01, reference_decay=1.0), iter_decay=0.5)
    aug = TrainAugment(erase=RandomMultiErasing([0.3, 0.6], 0.5, [0.1, 0.34]))

    def model():
        m = FeatRotationSymm(backbone_depth=18, num_iter=3)
        m.load_state_dict(sd, strict=True)
        m.input_size = None
        m.to(dev()).train()
        m.compute_dtype = torch.bfloat16
        return m

    def seed():
        torch.manual_seed(77), random.seed(77), np.random.seed(77)

    a = model()
    a.input_augment, a.input_bgr = aug, True
    seed()
    da = a(dict(rest, img_0=u8[0], img_1=u8[1]))
    assert bool(a._backbone._stem_rw) == stem_rw
    la = metrics(da)
    la.backward()
    seed()
    f32 = [aug.apply(u, aug.draw(B, hw, hw), out="nchw", bgr=True) for u in u8]
    b = model()
    db = b(dict(rest, img_0=f32[0], img_1=f32[1]))
    assert bool(b._backbone._stem_rw) == stem_rw
    lb = metrics(db)
    lb.backward()
    for k in ("pred_gaze", "img_feat_0", "img_feat_1", "_mvg_preds"):
        assert torch.equal(da[k], db[k]), k
    assert torch.equal(la, lb) and torch.isfinite(la)
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    with_grad = 0
    for k, p in pa.items():                             # (the backbone's unused fc layer has no gradient in either model)
        assert (p.grad is None) == (pb[k].grad is None), k
        if p.grad is not None:
            assert torch.equal(p.grad, pb[k].grad), k
            with_grad += 1
    assert with_grad >= len(pa) - 2 and with_grad > 60
    assert pa["_feat_extractor.0.conv1.weight"].grad.abs().max() > 0          # the stem's weight gradient read x0
    ba, bb = dict(a.named_buffers()), dict(b.named_buffers())
    moved = 0
    for k, v in ba.items():
        assert torch.equal(v, bb[k]), k
        moved += int("running_mean" in k and not torch.equal(v.cpu(), sd[k]))
    assert moved >= 10
    # without the augment object the raw bf16 training step is still refused
    a.input_augment = None
    with pytest.raises(NotImplementedError, match="inference only"):
        a(dict(rest, img_0=u8[0], img_1=u8[1]))
    # a patch of another size than input_size: refused, not resized
    a.input_augment, a.input_size = aug, 32
    with pytest.raises(ValueError, match="resize"):
        a(dict(rest, img_0=u8[0], img_1=u8[1]))
    a.input_size = None
    # eval mode: the attribute is ignored
    a.eval(), b.eval()
    b.input_bgr = True
    with torch.no_grad():
        ea = a(dict(rest, img_0=u8[0], img_1=u8[1]))
        eb = b(dict(rest, img_0=u8[0], img_1=u8[1]))
    assert torch.equal(ea["pred_gaze"], eb["pred_gaze"]) and torch.equal(ea["img_feat_1"], eb["img_feat_1"])
