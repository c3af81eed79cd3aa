"""Fine-tuning on the GPU: the segmented Adam step at kernel level (bit-equal to mvg_adam_step per slice, nothing touched outside
the segments), and the model with frozen parameters and parameter groups - which launches run, what the tape keeps, which
gradients exist, and the optimizer against a CPU torch.optim.Adam fed the same gradients.

Shapes: ResNet-18, 64 x 64 inputs, batch 4 (the build(18) / inputs(4, 64) size of test_model_gpu.py).  Bounds: torch.equal wherever
the same launches run on the same data (the kernels add their partial sums in a fixed order); the 2e-6 relative bound of
test_fused_adam_matches_torch_adam where the fused update is held against torch's."""
import contextlib

import numpy as np
import pytest
import torch

import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd import ops, synth

pytestmark = pytest.mark.gpu
BB = "_feat_extractor.0."
ADAM_TOL = 2e-6


def dev():
    return torch.device("cuda:0")


# ---------------------------------------------------------------- kernel level
def _arena(n, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g).to(dev())
    gr = (torch.randn(n, generator=g) * 0.1).to(dev())
    m = (torch.randn(n, generator=g) * 0.01).to(dev())
    v = (torch.rand(n, generator=g) * 1e-3).to(dev())
    return p, gr, m, v


def _check_segments(n, segs, seed=0):
    """Run the segmented step once; every slice must equal mvg_adam_step on that slice alone, everything else its old bits."""
    p, g, m, v = _arena(n, seed)
    before = [t.clone() for t in (p, m, v)]
    want = []
    for (b, e, lr, b1, b2, eps, wd, step) in segs:
        sl = [t[b:e].clone() for t in (p, g, m, v)]
        ops.adam_step(sl[0], sl[1], sl[2], sl[3], lr, b1, b2, eps, wd, step)
        want.append((sl[0], sl[2], sl[3]))
    ops.adam_step_segments(p, g, m, v, segs)
    torch.cuda.synchronize()
    outside = torch.ones(n, dtype=torch.bool, device=dev())
    for (b, e, *_), w in zip(segs, want):
        outside[b:e] = False
        for got, ref, what in zip((p, m, v), w, ("param", "exp_avg", "exp_avg_sq")):
            assert torch.equal(got[b:e], ref), f"{what} of segment [{b}, {e})"
        assert not torch.equal(p[b:e], before[0][b:e])               # (the step did move the slice)
    for got, old, what in zip((p, m, v), before, ("param", "exp_avg", "exp_avg_sq")):
        assert torch.equal(got[outside].view(torch.int32), old[outside].view(torch.int32)), f"{what} outside the segments"


def test_single_segment_equals_adam_step():
    n = 4096
    hyper = (1e-3, 0.9, 0.999, 1e-8, 1e-6, 3)
    p, g, m, v = _arena(n, 1)
    q = [t.clone() for t in (p, g, m, v)]
    ops.adam_step(p, g, m, v, *hyper)
    ops.adam_step_segments(q[0], q[1], q[2], q[3], [(0, n) + hyper])
    for a, b in zip((p, m, v), (q[0], q[2], q[3])):
        assert torch.equal(a, b)


def test_segments_with_holes_and_their_own_hyper_parameters():
    n = 4096
    _check_segments(n, [(0, 4, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1),                  # a 4-element segment starting at 0
                        (64, 1028, 1e-4, 0.8, 0.99, 1e-6, 1e-6, 5),
                        (2048, n, 5e-2, 0.5, 0.9, 1e-3, 1e-2, 100)])               # ... and one ending at n


def test_more_segments_than_one_launch_takes():
    rng = np.random.default_rng(3)
    segs, off = [], 0
    for i in range(35):                                                          # 16 + 16 + 3: three launches
        off += 4 * int(rng.integers(0, 5))                                       # holes of 0 .. 16 elements
        ln = 4 * int(rng.integers(1, 17))                                        # 4 .. 64 elements
        segs.append((off, off + ln, float(10.0 ** rng.uniform(-5, -2)), float(rng.uniform(0.5, 0.95)), float(rng.uniform(0.9, 0.9999)),
                     1e-8, float(rng.choice([0.0, 1e-6, 1e-2])), int(rng.integers(1, 50))))
        off += ln
    assert len(segs) == 35 and min(e - b for b, e, *_ in segs) >= 4 and max(e - b for b, e, *_ in segs) <= 64
    _check_segments(off + 64, segs)


def test_grid_stride_loop_over_the_concatenated_length():
    cap = 8192 * 256 * 4                                                         # the grid cap times 4 elements per lane
    a = 5_000_000
    segs = [(1024, 1024 + a, 1e-3, 0.9, 0.999, 1e-8, 1e-6, 2),
            (1024 + a + 4096, 1024 + a + 4096 + (cap - a) + 512, 1e-4, 0.8, 0.99, 1e-8, 0.0, 7)]
    assert sum(e - b for b, e, *_ in segs) == cap + 512
    _check_segments(segs[-1][1] + 2048, segs)


@pytest.mark.parametrize("name,segs", [
    ("unsorted", [(64, 128, 1), (0, 32, 1)]),
    ("overlap", [(0, 64, 1), (32, 96, 1)]),
    ("aligned", [(2, 66, 1)]),
    ("outside", [(0, 64, 1), (4000, 4100, 1)]),
    ("step", [(0, 64, 1), (128, 256, 0)]),
    ("empty", [(64, 64, 1)]),
])
def test_bad_segments_are_rejected_before_any_launch(name, segs):
    n = 4096
    p, g, m, v = _arena(n, 2)
    before = [t.clone() for t in (p, m, v)]
    with pytest.raises(RuntimeError, match="adam_step_segments: .*" + name):
        ops.adam_step_segments(p, g, m, v, [(b, e, 1e-3, 0.9, 0.999, 1e-8, 0.0, s) for b, e, s in segs])
    torch.cuda.synchronize()
    for got, old in zip((p, m, v), before):                                      # the valid first segment was not run either
        assert torch.equal(got, old)


# ---------------------------------------------------------------- model level
_SD = {}


def build(train=True, bf16=False):
    from rot_mvgaze_amd.model import FeatRotationSymm
    if not _SD:
        _SD.update({k: torch.from_numpy(np.array(v)) for k, v in synth.make_state_dict(18, 0, 3, perturb_bn=True).items()})
    m = FeatRotationSymm(backbone_depth=18, num_iter=3)
    m.load_state_dict(_SD, strict=True)
    m.to(dev())
    if bf16:
        m.compute_dtype = torch.bfloat16
    return m.train() if train else m.eval()


def inputs(seed=1234):
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    inp = synth.make_inputs(4, 2, seed, 64)
    img, hp, gt = (torch.from_numpy(inp[k]).to(dev()) for k in ("img", "head_pose", "gt_gaze"))
    return {"img_0": img[:, 0].contiguous(), "img_1": img[:, 1].contiguous(),
            "rot_0": rotation_matrix_2d(hp[:, 0].contiguous()), "rot_1": rotation_matrix_2d(hp[:, 1].contiguous()),
            "gt_gaze": gt[:, 0].contiguous(), "gt_gaze_1": gt[:, 1].contiguous()}


def metrics():
    from rot_mvgaze_amd.losses import IterationLoss, StereoL1Loss
    return IterationLoss(StereoL1Loss(rel_weight=0.01, reference_decay=1.0, distance_metric="angular_error",
                                      pred_gaze_key="pred_gaze"), iter_decay=0.5)


def rel_close(got, ref, tol, what):
    got = got.detach().cpu().double().numpy()
    ref = ref.detach().cpu().double().numpy()
    err, scale = np.abs(got - ref).max(), np.abs(ref).max() + 1e-30
    assert err <= tol * scale, f"{what}: max err {err:.3e}, scale {scale:.3e}, rel {err / scale:.3e}"


def freeze(m, pred):
    names = [k for k, p in m.named_parameters() if pred(k)]
    for k, p in m.named_parameters():
        if pred(k):
            p.requires_grad_(False)
    assert names
    return set(names)


def in_prefix(name):
    """The stem, layer1 and layer2 (a parameter's name or a unit's)."""
    return name.startswith(BB) and ".fc." not in name and ".layer3." not in name and ".layer4." not in name


def is_bn_affine(name):
    return name.startswith(BB) and (".bn" in name or ".downsample.1." in name)


def backward(m, seed=1234):
    """One forward + loss + backward from empty gradients.  Returns (gradients by name, bytes the forward left allocated)."""
    for p in m.parameters():
        p.grad = None
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    loss = metrics()(m(inputs(seed)))
    held = torch.cuda.memory_allocated() - before
    loss.backward()
    torch.cuda.synchronize()
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}, held


@contextlib.contextmanager
def launch_spy():
    """(method, unit name) of every Backbone._wgrad / _dgrad / _bn_bwd / _stem_bn_bwd call."""
    from rot_mvgaze_amd.backbone import Backbone
    calls, saved = [], {}
    for name in ("_wgrad", "_dgrad", "_bn_bwd", "_stem_bn_bwd"):
        saved[name] = orig = getattr(Backbone, name)

        def wrapped(self, u, *a, _orig=orig, _name=name, **kw):
            calls.append((_name, u.spec.name))
            return _orig(self, u, *a, **kw)
        setattr(Backbone, name, wrapped)
    try:
        yield calls
    finally:
        for name, orig in saved.items():
            setattr(Backbone, name, orig)


_REF = {}


def unfrozen(mode):
    """The gradients (and forward bytes, running statistics) of the step with nothing frozen, once per mode."""
    if mode not in _REF:
        m = build(train=mode != "eval", bf16=mode == "bf16")
        with launch_spy() as calls:
            grads, held = backward(m)
        _REF[mode] = (grads, held, {k: b.detach().clone() for k, b in m.named_buffers()}, list(calls))
    return _REF[mode]


def _same_gradients(got, ref, frozen):
    assert set(got) == set(ref) - frozen
    for k, g in got.items():
        assert torch.equal(g, ref[k]), k


def _cpu_twin(m, groups_of_names=None, **defaults):
    """CPU leaves of every parameter and a torch.optim.Adam over them with the same groups."""
    ref_p = {k: p.detach().cpu().clone().contiguous().requires_grad_(True) for k, p in m.named_parameters()}
    if groups_of_names is None:
        return ref_p, torch.optim.Adam(list(ref_p.values()), **defaults)
    return ref_p, torch.optim.Adam([dict(g, params=[ref_p[k] for k in g["params"]]) for g in groups_of_names], **defaults)


def _feed(m, ref_p):
    for k, p in m.named_parameters():
        ref_p[k].grad = None if p.grad is None else p.grad.detach().cpu().contiguous().clone()


def test_head_only_step_leaves_the_backbone_alone(monkeypatch):
    from rot_mvgaze_amd.optim import Adam
    m = build()
    opt = Adam(m.parameters(), lr=1e-3, weight_decay=1e-6)
    ref_p, ref_opt = _cpu_twin(m, lr=1e-3, weight_decay=1e-6)
    # step 1 with everything trainable, so that the backbone has moments worth keeping
    backward(m, seed=10)
    _feed(m, ref_p)
    opt.step()
    ref_opt.step()
    frozen = freeze(m, lambda k: k.startswith("_feat_extractor"))
    for k in frozen:
        ref_p[k].requires_grad_(False)
    opt.zero_grad()
    ref_opt.zero_grad()
    st = opt._flat[id(m)]
    arena, entries = m.grad_arena()
    snap = [t.clone() for t in (m.param_arena(), st["exp_avg"], st["exp_avg_sq"])]
    seen = []
    real = ops.adam_step_segments
    monkeypatch.setattr(ops, "adam_step_segments", lambda p, g, a, b, segs: (seen.append(list(segs)), real(p, g, a, b, segs))[1])
    with launch_spy() as calls:
        grads, _ = backward(m, seed=11)
    assert not calls                                                 # no backbone backward at all
    assert not any(k in frozen for k in grads)
    _feed(m, ref_p)
    opt.step()
    ref_opt.step()
    torch.cuda.synchronize()
    assert len(seen) == 1 and len(seen[0]) == 1                      # the head and the lifter: one segment
    names = {id(p): k for k, p in m.named_parameters()}
    for (p, off, n) in entries:
        if names[id(p)] in frozen:
            assert p.grad is None
            for now, old in zip((m.param_arena(), st["exp_avg"], st["exp_avg_sq"]), snap):
                assert torch.equal(now[off:off + n].view(torch.int32), old[off:off + n].view(torch.int32)), names[id(p)]
        else:
            rel_close(p, ref_p[names[id(p)]], ADAM_TOL, "param after the head-only step " + names[id(p)])
    begin, end = seen[0][0][0:2]
    assert begin == 0 and end == min(off for (p, off, n) in entries if names[id(p)] in frozen)
    assert [s for (p, _, _), s in zip(entries, st["steps"]) if names[id(p)] in frozen] == [1] * (len(frozen) - 2)   # (resnet.fc: no arena slot)
    assert {s for (p, _, _), s in zip(entries, st["steps"]) if names[id(p)] not in frozen} == {2}


def _below_boundary_is_silent(calls):
    assert calls
    assert [c for c in calls if in_prefix(c[1])] == []
    # the boundary block (layer3.0) hands no gradient down: its conv1 and its downsample branch run no backward-data
    assert [c for c in calls if c[0] == "_dgrad" and c[1] in (BB + "layer3.0.conv1", BB + "layer3.0.downsample.0")] == []
    assert ("_wgrad", BB + "layer3.0.conv1") in calls and ("_wgrad", BB + "layer3.0.downsample.0") in calls


def test_frozen_prefix_with_two_groups():
    from rot_mvgaze_amd.optim import Adam
    ref_grads, ref_held, ref_buffers, ref_calls = unfrozen("train")
    assert [c for c in ref_calls if in_prefix(c[1])] and ("_stem_bn_bwd", BB + "conv1") in ref_calls
    m = build()
    frozen = freeze(m, in_prefix)
    m._debug_keep_tapes = True
    with launch_spy() as calls:
        grads, held = backward(m)
    _same_gradients(grads, ref_grads, frozen)
    for k, b in m.named_buffers():                                   # the forward ran as ever: batch statistics everywhere
        assert torch.equal(b, ref_buffers[k]), k
    _below_boundary_is_silent(calls)
    # the tape: nothing of the units below the boundary; the boundary block still has its input
    m._debug_keep_tapes = False
    for p in m.parameters():
        p.grad = None
    m._debug_keep_tapes = True
    loss = metrics()(m(inputs()))
    tape = m._last_backbone_tape
    assert tape["boundary"] == 4                                     # ResNet-18: layer3.0 is the fifth block
    for u in tape["units"]:
        kept = [f for f in ("x_in", "y", "out", "mean", "invstd", "w", "pool", "relu_affine", "relu_bits") if getattr(u, f) is not None]
        if in_prefix(u.spec.name):
            assert kept == [], (u.spec.name, kept)
        else:
            assert "x_in" in kept and "y" in kept, (u.spec.name, kept)
    del tape, loss
    m._last_backbone_tape = None
    m._debug_keep_tapes = False
    assert held < ref_held                                           # and the forward holds fewer bytes for the backward
    # three steps of the two-group optimizer against torch's
    def names(pred):
        return [k for k, p in m.named_parameters() if pred(k)]
    groups = [{"params": names(lambda k: ".layer3." in k or ".layer4." in k), "lr": 1e-4, "weight_decay": 1e-6},
              {"params": names(lambda k: not k.startswith("_feat_extractor")), "lr": 1e-3, "weight_decay": 0.0}]
    byname = dict(m.named_parameters())
    opt = Adam([dict(g, params=[byname[k] for k in g["params"]]) for g in groups])
    ref_p, ref_opt = _cpu_twin(m, groups)
    start = {k: p.detach().clone() for k, p in m.named_parameters()}
    for it in range(3):
        backward(m, seed=20 + it)
        _feed(m, ref_p)
        opt.step()
        ref_opt.step()
    for k, p in m.named_parameters():
        if k in frozen or ".fc." in k:
            assert p.grad is None and torch.equal(p.detach(), start[k]), k
        else:
            rel_close(p, ref_p[k], ADAM_TOL, "param after three grouped steps " + k)
            assert not torch.equal(p.detach(), start[k]), k


def test_holes_above_the_boundary():
    from rot_mvgaze_amd.optim import Adam
    ref_grads, _, _, _ = unfrozen("train")
    conv = BB + "layer4.1.conv1"
    m = build()
    frozen = freeze(m, lambda k: is_bn_affine(k) or k == conv + ".weight")
    assert len(frozen) == 2 * 20 + 1                                 # ResNet-18: 20 BatchNorm layers
    with launch_spy() as calls:
        grads, _ = backward(m)
    _same_gradients(grads, ref_grads, frozen)
    wgrads = [c[1] for c in calls if c[0] == "_wgrad"]
    assert conv not in wgrads and len(wgrads) == 19                  # every other conv, the stem included
    assert ("_dgrad", conv) in calls                                 # its backward-data runs as before
    start = {k: p.detach().clone() for k, p in m.named_parameters()}
    opt = Adam(m.parameters(), lr=1e-3)
    opt.step()
    torch.cuda.synchronize()
    for k, p in m.named_parameters():
        if k in frozen:
            assert p.grad is None and torch.equal(p.detach(), start[k]), k
        elif ".fc." not in k:
            assert not torch.equal(p.detach(), start[k]), k


def test_unfreeze_schedule_and_checkpoint():
    from rot_mvgaze_amd.optim import Adam
    m = build()
    opt = Adam(m.parameters(), lr=1e-3, weight_decay=1e-6)
    ref_p, ref_opt = _cpu_twin(m, lr=1e-3, weight_decay=1e-6)
    frozen = freeze(m, lambda k: k.startswith("_feat_extractor"))
    for it in range(2):                                              # steps 1 - 2: the head alone
        backward(m, seed=30 + it)
        _feed(m, ref_p)
        opt.step()
        ref_opt.step()
    for k, p in m.named_parameters():
        p.requires_grad_(True)
    backward(m, seed=32)                                             # step 3: everything
    _feed(m, ref_p)
    sd = opt.state_dict()
    assert sorted(set(sd["mvg_arena_state"][0]["steps"])) == [0, 2] and sd["mvg_arena_state"][0]["step"] == 2
    at2 = m.param_arena().clone()
    opt.step()
    ref_opt.step()
    torch.cuda.synchronize()
    assert sorted(set(opt._flat[id(m)]["steps"])) == [1, 3]          # the backbone's bias correction starts at 1
    for k, p in m.named_parameters():
        if ".fc." not in k:
            rel_close(p, ref_p[k], ADAM_TOL, "param after the unfreeze schedule " + k)
    straight = m.param_arena().clone()
    # the same third step from the checkpoint taken after step 2: a fresh optimizer, the same gradients
    m.param_arena().copy_(at2)
    opt2 = Adam(m.parameters(), lr=1e-3, weight_decay=1e-6)
    opt2.load_state_dict(sd)
    opt2.step()
    torch.cuda.synchronize()
    assert torch.equal(m.param_arena(), straight)
    assert opt2._flat[id(m)]["steps"] == opt._flat[id(m)]["steps"]
    for a, b in ((opt._flat[id(m)][key], opt2._flat[id(m)][key]) for key in ("exp_avg", "exp_avg_sq")):
        assert torch.equal(a, b)


@pytest.mark.parametrize("mode", ["eval", "bf16"])
def test_frozen_prefix_in_eval_mode_and_on_the_bf16_path(mode):
    ref_grads, ref_held, _, _ = unfrozen(mode)
    m = build(train=mode != "eval", bf16=mode == "bf16")
    frozen = freeze(m, in_prefix)
    with launch_spy() as calls:
        grads, held = backward(m)
    _same_gradients(grads, ref_grads, frozen)
    _below_boundary_is_silent(calls)
    assert held < ref_held


def test_data_parallel_refuses_frozen_parameters():
    from rot_mvgaze_amd.dp import GradAllReducer
    m = build()
    freeze(m, lambda k: k == BB + "conv1.weight")
    try:
        with pytest.raises(NotImplementedError, match="frozen parameters"):
            GradAllReducer(m, force=True, broadcast=False)
        assert m._on_grads_ready is None and m._on_backward_done is None
        # ... and one frozen after construction is refused by the first backward
        m2 = build()
        GradAllReducer(m2, force=True, broadcast=False)
        freeze(m2, lambda k: k == BB + "conv1.weight")
        with pytest.raises(NotImplementedError, match="frozen parameters"):
            metrics()(m2(inputs())).backward()
    finally:
        ops.set_reserved_cus(0)


def test_capturable_refuses_a_skipped_parameter_at_step():
    from rot_mvgaze_amd.optim import Adam
    m = build()
    opt = Adam(m.parameters(), lr=1e-3, capturable=True)
    freeze(m, lambda k: k.startswith("_feat_extractor"))
    backward(m)
    before = m.param_arena().clone()
    with pytest.raises(NotImplementedError, match="capturable=True.*at step"):
        opt.step()
    torch.cuda.synchronize()
    assert torch.equal(m.param_arena(), before)                      # refused before anything was updated


def test_one_group_nothing_frozen_is_the_one_launch_of_before(monkeypatch):
    from rot_mvgaze_amd.optim import Adam
    m = build()
    opt = Adam(m.parameters(), lr=1e-3, weight_decay=1e-6)
    seen = []
    real_step, real_segments = ops.adam_step, ops.adam_step_segments
    monkeypatch.setattr(ops, "adam_step", lambda *a: (seen.append(("adam_step", a[4:])), real_step(*a))[1])
    monkeypatch.setattr(ops, "adam_step_segments", lambda *a: (seen.append(("adam_step_segments",)), real_segments(*a))[1])
    for it in range(2):
        backward(m, seed=40 + it)
        opt.step()
    assert seen == [("adam_step", (1e-3, 0.9, 0.999, 1e-8, 1e-6, 1)), ("adam_step", (1e-3, 0.9, 0.999, 1e-8, 1e-6, 2))]
