"""TrainAugment(draws="device") on the GPU: mvg_augment_draw writes, bit for bit, the records, masks and grid sizes of the
NumPy restatement (tests/augment_draw_ref.py); the pixel launches read them as they read host draws; a model step, and a
captured step (graph.GraphedStep) on raw uint8 patches, equal the steps fed the restated draws; the eager step does not
synchronise the host."""
import numpy as np
import pytest
import torch

import augment_draw_ref as R
import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd import ops, synth
from rot_mvgaze_amd.augment import REC_DTYPE, AugmentDraws, DeviceDraws, RandomMultiErasing, TrainAugment

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE1234567890                               # the high word is set
ERASE = dict(p=0.5, proportion=(0.5, 0.6), dot_size=(0.05, 0.3))
SMALL_ERASE = dict(p=0.7, proportion=(0.3, 0.6), dot_size=(0.1, 0.34))       # a 10 x 10 grid at most: coarse on small patches
CONFIGS = {"recipe": dict(R.RECIPE),
           "no_erase": dict(R.RECIPE, erase=None),
           "factors_off": dict(R.RECIPE, brightness=0.0, contrast=0.0, saturation=0.0),
           "no_translate": dict(R.RECIPE, translate=None),
           "no_scale": dict(R.RECIPE, scale=None),
           "p0": dict(R.RECIPE, erase=dict(ERASE, p=0.0)),
           "p1": dict(R.RECIPE, erase=dict(ERASE, p=1.0))}


def dev():
    return torch.device("cuda:0")


def make_augment(settings, seed=SEED):
    e = settings["erase"]
    erase = None if e is None else RandomMultiErasing(list(e["proportion"]), e["p"], list(e["dot_size"]))
    return TrainAugment(**dict(settings, erase=erase), draws="device", seed=seed)


def restated(n, h, w, seed, counter, settings):
    """The restatement's draws as the AugmentDraws the host path takes."""
    recs, masks, grid, _ = R.draw(n, h, w, seed, counter, **settings)
    if masks is None:
        return AugmentDraws(recs, None)
    return AugmentDraws(recs, [(int(g), torch.from_numpy(masks[i, : g * g].reshape(g, g).copy())) for i, g in enumerate(grid)])


def raw_launch(aug, n, h, w, counter):
    """ops.augment_draw into destinations prefilled with 0xFF bytes -> (recs, masks, grid) as numpy."""
    d = dev()
    gmax = aug._gmax
    recs = torch.full((n * 56,), 0xFF, dtype=torch.uint8, device=d)
    masks = grid = None
    if aug.erase is not None:
        masks = torch.full((n * gmax * gmax * 4,), 0xFF, dtype=torch.uint8, device=d).view(torch.float32).reshape(n, gmax * gmax)
        grid = torch.full((n * 4,), 0xFF, dtype=torch.uint8, device=d).view(torch.int32)
    ops.augment_draw(recs, masks, grid, gmax, n, h, w, aug._draw_cfg(h, w), aug.seed, counter)
    torch.cuda.synchronize()
    return (recs.cpu().numpy().view(REC_DTYPE), None if masks is None else masks.cpu().numpy(), None if grid is None else grid.cpu().numpy())


@pytest.mark.parametrize("name", list(CONFIGS))
def test_buffers_equal_the_restatement_bit_for_bit(name):
    settings = CONFIGS[name]
    aug = make_augment(settings)
    counter = torch.full((1,), 5, dtype=torch.int64, device=dev())
    k = 5
    erased = kept = 0
    for n in (1, 5, 67):
        for h, w in ((8, 8), (17, 23), (224, 224)):
            recs, masks, grid = raw_launch(aug, n, h, w, counter)
            want_recs, want_masks, want_grid, _ = R.draw(n, h, w, SEED, k, **settings)
            k += 1
            assert recs.tobytes() == want_recs.tobytes(), (n, h, w)
            if settings["erase"] is None:
                assert masks is None and grid is None and want_masks is None
                continue
            assert grid.tobytes() == want_grid.tobytes() and masks.tobytes() == want_masks.tobytes(), (n, h, w)
            erased += int((grid > 0).sum())
            kept += int(masks.sum())
    assert int(counter.item()) == k == 14
    if name == "p0":                                    # u > 0 fails only for a zero word: all 219 images are left alone
        assert erased == 0 and kept == 0
    elif name == "p1":
        assert erased == 3 * (1 + 5 + 67)
    elif settings["erase"] is not None:
        assert 0 < erased < 3 * (1 + 5 + 67) and kept > 0


def test_counter_crosses_into_its_high_word():
    aug = make_augment(CONFIGS["recipe"])
    aug.load_state_dict({"seed": SEED, "counter": (1 << 32) - 1})          # before the first launch: the counter starts there
    seen = []
    for k in range(3):
        d = aug.draw_device(5, 17, 23, dev())
        assert isinstance(d, DeviceDraws) and d.gmax == 20 and d.masks.shape == (5, 400) and d.grid.shape == (5,)
        want_recs, want_masks, want_grid, _ = R.draw(5, 17, 23, SEED, (1 << 32) - 1 + k, **CONFIGS["recipe"])
        assert d.recs.cpu().numpy().view(REC_DTYPE).tobytes() == want_recs.tobytes(), k
        assert d.masks.cpu().numpy().tobytes() == want_masks.tobytes() and d.grid.cpu().numpy().tobytes() == want_grid.tobytes(), k
        seen.append(want_recs.tobytes())
    assert len(set(seen)) == 3
    assert aug.state_dict() == {"seed": SEED, "counter": (1 << 32) + 2}
    ptr = aug._counter.data_ptr()
    aug.load_state_dict({"seed": SEED, "counter": (1 << 32) - 1})          # in place: the first launch again
    assert aug._counter.data_ptr() == ptr
    assert aug.draw_device(5, 17, 23, dev()).recs.cpu().numpy().tobytes() == seen[0]
    with pytest.raises(ValueError, match="seed"):
        aug.load_state_dict({"seed": SEED + 1, "counter": 0})


def test_pixel_launches_read_device_draws_as_host_draws():
    """n = 3, 16 x 24, stored BGR: apply with a DeviceDraws == apply with its to_host() draws, every destination form."""
    rng = np.random.RandomState(3)
    u8 = torch.from_numpy(rng.randint(0, 256, (3, 16, 24, 3)).astype(np.uint8)).to(dev())
    settings = dict(R.RECIPE, erase=SMALL_ERASE)
    aug = make_augment(settings)
    d = aug.draw_device(3, 16, 24, dev())
    host = d.to_host()
    want = restated(3, 16, 24, SEED, 0, settings)
    assert host.recs.tobytes() == want.recs.tobytes() and [g for g, _ in host.erase] == [g for g, _ in want.erase]
    assert all(torch.equal(a[1], b[1]) for a, b in zip(host.erase, want.erase))
    assert any(g for g, _ in host.erase) and any(g and 0 < float(m.sum()) < g * g for g, m in host.erase)      # an erase that shows
    plain = aug.apply(u8, AugmentDraws(host.recs, None), out="nhwc4", bgr=True)
    for out in ("nhwc4", "nchw", "nhwc8_bf16", "rw_bf16"):
        got, ref = aug.apply(u8, d, out=out, bgr=True), aug.apply(u8, host, out=out, bgr=True)
        assert got.dtype == ref.dtype and torch.equal(got, ref), out
    assert not torch.equal(aug.apply(u8, d, out="nhwc4", bgr=True), plain)
    with pytest.raises(ValueError, match="out='u8' needs erase=None"):
        aug.apply(u8, d, out="u8", bgr=True)
    with pytest.raises(ValueError, match="records"):
        aug.apply(u8[:2], d, out="nhwc4", bgr=True)
    bare = make_augment(dict(R.RECIPE, erase=None))
    d = bare.draw_device(3, 16, 24, dev())
    assert d.masks is None and d.grid is None and d.gmax == 0 and d.to_host().erase is None
    got = bare.apply(u8, d, out="u8", bgr=True)
    assert got.dtype == torch.uint8 and torch.equal(got, bare.apply(u8, d.to_host(), out="u8", bgr=True))
    assert not torch.equal(got, u8.flip(-1))
    # __call__ follows the mode: the next launch of the object
    assert torch.equal(bare(u8, out="u8", bgr=True), bare.apply(u8, restated(3, 16, 24, SEED, 1, dict(R.RECIPE, erase=None)), out="u8", bgr=True))
    torch.cuda.synchronize()


def _dict_step_setup(B, hw):
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    from rot_mvgaze_amd.losses import IterationLoss, StereoL1Loss
    rng = np.random.RandomState(9)
    u8 = [torch.from_numpy(rng.randint(0, 256, (B, hw, hw, 3)).astype(np.uint8)).to(dev()) for _ in range(2)]
    inp = synth.make_inputs(B, 2, 1234, hw)
    hp, gt = (torch.from_numpy(inp[k]).to(dev()) for k in ("head_pose", "gt_gaze"))
    rest = {"rot_0": rotation_matrix_2d(hp[:, 0].contiguous()), "rot_1": rotation_matrix_2d(hp[:, 1].contiguous()),
            "gt_gaze": gt[:, 0].contiguous(), "gt_gaze_1": gt[:, 1].contiguous()}
    sd = {k: torch.from_numpy(np.array(v)) for k, v in synth.make_state_dict(18, 0, 3, perturb_bn=True).items()}
    metrics = IterationLoss(StereoL1Loss(rel_weight=0.01, reference_decay=1.0), iter_decay=0.5)
    return u8, rest, sd, metrics


@pytest.mark.parametrize("bf16,stem_rw", [(False, True), (True, True), (True, False)], ids=["fp32", "bf16_row_windows", "bf16_nhwc8"])
def test_model_step_with_device_draws(bf16, stem_rw):
    """ResNet-18, V=2, B=2, 64 x 64 BGR uint8 patches, train mode: a step with a device-draw input_augment equals a step of
    the same weights fed TrainAugment.apply(out="nchw") of the restated draws (launch v of the object draws view v) - outputs,
    loss, every gradient and every buffer, bit for bit."""
    from rot_mvgaze_amd.model import FeatRotationSymm
    B, hw = 2, 64
    u8, rest, sd, metrics = _dict_step_setup(B, hw)
    settings = dict(R.RECIPE, erase=SMALL_ERASE)
    aug = make_augment(settings)

    def model():
        m = FeatRotationSymm(backbone_depth=18, num_iter=3)
        m.load_state_dict(sd, strict=True)
        m.input_size = None
        m.to(dev()).train()
        if bf16:
            m.compute_dtype = torch.bfloat16
        m.ensure_layout()
        m._backbone.stem_rowwindow = stem_rw            # the stem's other form at the same shapes
        return m

    a = model()
    a.input_augment, a.input_bgr = aug, True
    da = a(dict(rest, img_0=u8[0], img_1=u8[1]))
    assert not bf16 or bool(a._backbone._stem_rw) == stem_rw
    la = metrics(da)
    la.backward()
    assert aug.state_dict()["counter"] == 2
    draws = [restated(B, hw, hw, SEED, v, settings) for v in range(2)]
    assert any(g for d in draws for g, _ in d.erase)
    f32 = [aug.apply(u, d, out="nchw", bgr=True) for u, d in zip(u8, draws)]
    b = model()
    db = b(dict(rest, img_0=f32[0], img_1=f32[1]))
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
    ba, bb = dict(a.named_buffers()), dict(b.named_buffers())
    moved = 0
    for k, v in ba.items():
        assert torch.equal(v, bb[k]), k
        moved += int("running_mean" in k and not torch.equal(v.cpu(), sd[k]))
    assert moved >= 10


def _graph_setup(bf16, B=2, V=2, hw=64):
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    from rot_mvgaze_amd.losses import MultiViewIterationLoss
    from rot_mvgaze_amd.model import MultiViewGaze
    from rot_mvgaze_amd.optim import Adam
    m = MultiViewGaze(18, 3)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.make_state_dict(18, 0, 3).items()}, strict=True)
    m.to(dev()).train()
    if bf16:
        m.compute_dtype = torch.bfloat16
    aug = make_augment(dict(R.RECIPE, erase=SMALL_ERASE))
    m.input_augment, m.input_bgr, m.input_size = aug, True, None
    rng = np.random.RandomState(21)
    img = [torch.from_numpy(rng.randint(0, 256, (B, hw, hw, 3)).astype(np.uint8)).to(dev()) for _ in range(V)]      # static raw inputs
    inp = synth.make_inputs(B, V, 77, hw)
    gt = torch.from_numpy(inp["gt_gaze"]).to(dev())
    rot = rotation_matrix_2d(torch.from_numpy(inp["head_pose"]).reshape(-1, 2).to(dev())).reshape(B, V, 3, 3)
    crit = MultiViewIterationLoss(rel_weight=0.01, reference_decay=1.0, iter_decay=0.5)
    opt = Adam(m.parameters(), lr=1e-3, weight_decay=1e-6, capturable=True)

    def step():
        m.zero_grad(set_to_none=True)
        loss = crit(m.forward_multiview(img, rot), gt)
        loss.backward()
        opt.step()
        return loss
    return m, opt, aug, step


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_captured_step_on_raw_patches_replays_the_eager_step(bf16):
    from rot_mvgaze_amd.graph import GraphedStep
    warm, n, V = 2, 3, 2
    m1, o1, a1, s1 = _graph_setup(bf16)
    for _ in range(warm):
        s1()
    eager_losses = [float(s1().item()) for _ in range(n)]
    m2, o2, a2, s2 = _graph_setup(bf16)
    gs = GraphedStep(m2, s2, o2, warmup=warm)
    assert a2.state_dict()["counter"] == V * warm                   # the capture itself draws nothing
    ptr = a2._counter.data_ptr()
    graph_losses = []
    for k in range(n):
        graph_losses.append(float(gs.run().item()))
        assert a2.state_dict()["counter"] == V * (warm + k + 1)       # V launches per replay
    assert graph_losses == eager_losses, (graph_losses, eager_losses)
    assert len(set(graph_losses)) == n
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    for k in sd1:
        assert torch.equal(sd1[k], sd2[k]), k
    assert a1.state_dict() == a2.state_dict() == {"seed": SEED, "counter": V * (warm + n)}
    # with the learning rate at zero the parameters stand still and the inputs are unchanged: only the draws move the loss
    o2.param_groups[0]["lr"] = 0.0
    first, second = float(gs.run().item()), float(gs.run().item())
    assert first != second
    # load_state_dict between replays takes effect, in place: back to the counter of the replay before
    a2.load_state_dict({"seed": SEED, "counter": V * (warm + n + 1)})
    assert a2._counter.data_ptr() == ptr
    assert float(gs.run().item()) == second
    assert a2.state_dict()["counter"] == V * (warm + n + 2)


def test_device_draw_step_does_not_synchronise_the_host():
    """The method of test_model_gpu.py::test_training_step_does_not_synchronise_the_host on the eager step from raw patches."""
    from rot_mvgaze_amd.model import FeatRotationSymm
    from rot_mvgaze_amd.optim import Adam
    u8, rest, sd, metrics = _dict_step_setup(2, 64)
    m = FeatRotationSymm(backbone_depth=18, num_iter=3)
    m.load_state_dict(sd, strict=True)
    m.input_size = None
    m.to(dev()).train()
    aug = make_augment(dict(R.RECIPE, erase=SMALL_ERASE))
    m.input_augment, m.input_bgr = aug, True
    opt = Adam(m.parameters(), lr=1e-4, weight_decay=1e-6)
    d = dict(rest, img_0=u8[0], img_1=u8[1])

    def step():
        opt.zero_grad()
        metrics(m(dict(d))).backward()
        opt.step()
    step()                                              # first call: arenas, index tensors, scratch buffers, the launch counter
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        step()
        step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert aug.state_dict()["counter"] == 6
