"""A fine-tuning step - frozen parameters, parameter groups, frozen BatchNorm - captured in a hipGraph: optim.Adam(capturable="segments")
keeps one learning rate per group and one step counter per segment on the device (mvg_adam_step_segments_dev), and
graph.GraphedStep replays the step to the bits of the eager step.

Shapes: ResNet-18, V=2, B=4, 64 px unless said otherwise; weights and inputs are synth's, built the way test_graph_gpu._setup builds
them.  Bounds: torch.equal wherever the same launches run on the same data (replay against eager); rtol 2e-6 / atol 1e-8 where the
device-resident step is held against the host-side one (the bar of test_graph_gpu.test_device_side_adam_is_the_host_side_adam: the
two differ in where lr / bias-correction scalars are formed)."""
import numpy as np
import pytest
import torch

from rot_mvgaze_amd import synth

pytestmark = pytest.mark.gpu
BB = "_feat_extractor.0."
LRS = [(1e-3, 1e-4), (5e-4, 2e-4), (2e-3, 1e-5)]          # (head, backbone) learning rates, moved between steps
_SD = {}


def dev():
    return torch.device("cuda:0")


def in_prefix(name):
    """The stem, layer1 and layer2."""
    return name.startswith(BB) and ".fc." not in name and ".layer3." not in name and ".layer4." not in name


def up_to_layer1(name):
    return in_prefix(name) and ".layer2." not in name


def is_bn_affine(name):
    return name.startswith(BB) and (".bn" in name or ".downsample.1." in name)


def _setup(depth=18, V=2, B=4, hw=64, capturable="segments", bf16=False, frozen=in_prefix, groups=True, freeze_bn=False):
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    from rot_mvgaze_amd.losses import MultiViewIterationLoss
    from rot_mvgaze_amd.model import MultiViewGaze
    from rot_mvgaze_amd.optim import Adam
    if depth not in _SD:
        _SD[depth] = {k: torch.from_numpy(np.array(v)) for k, v in synth.make_state_dict(depth, 0, 3).items()}
    m = MultiViewGaze(depth, 3)
    m.load_state_dict(_SD[depth], strict=True)
    m.to(dev()).train()
    if bf16:
        m.compute_dtype = torch.bfloat16
    if freeze_bn:
        m.freeze_batchnorm = True
    for k, p in m.named_parameters():
        if (frozen is not None and frozen(k)) or (freeze_bn and is_bn_affine(k)):
            p.requires_grad_(False)
    inp = synth.make_inputs(B, V, 77, hw)
    img = [torch.from_numpy(np.ascontiguousarray(inp["img"][:, v])).to(dev()) for v in range(V)]
    gt = torch.from_numpy(inp["gt_gaze"]).to(dev())
    rot = rotation_matrix_2d(torch.from_numpy(inp["head_pose"]).reshape(-1, 2).to(dev())).reshape(B, V, 3, 3)
    crit = MultiViewIterationLoss(rel_weight=0.01, reference_decay=1.0, iter_decay=0.5)
    if groups:
        head = [p for k, p in m.named_parameters() if not k.startswith("_feat_extractor")]
        bb = [p for k, p in m.named_parameters() if k.startswith("_feat_extractor")]
        opt = Adam([{"params": head, "lr": 1e-3, "weight_decay": 0.0}, {"params": bb, "lr": 1e-4, "weight_decay": 1e-6}], capturable=capturable)
    else:
        opt = Adam(m.parameters(), lr=1e-3, weight_decay=1e-6, capturable=capturable)

    def step(optimize=True):
        m.zero_grad(set_to_none=True)
        loss = crit(m.forward_multiview(img, rot), gt)
        loss.backward()
        if optimize:
            opt.step()
        return loss
    return m, opt, step


def _set_lrs(opt, lrs):
    for g, lr in zip(opt.param_groups, lrs):
        g["lr"] = lr


def _arena_names(m):
    names = {id(p): k for k, p in m.named_parameters()}
    return [names[id(p)] for (p, _, _) in m.grad_arena()[1]]


def _steps(m, opt):
    """Per-parameter step counts by name, from the checkpoint (which reads the device table)."""
    (entry,) = opt.state_dict()["mvg_arena_state"]
    assert entry["step"] == max(entry["steps"])
    return dict(zip(_arena_names(m), entry["steps"]))


def _same_state(m1, o1, m2, o2):
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    for k in sd1:
        assert torch.equal(sd1[k], sd2[k]), k
    (e1,), (e2,) = o1.state_dict()["mvg_arena_state"], o2.state_dict()["mvg_arena_state"]
    assert e1["steps"] == e2["steps"] and e1["step"] == e2["step"]
    assert torch.equal(e1["exp_avg"], e2["exp_avg"]) and torch.equal(e1["exp_avg_sq"], e2["exp_avg_sq"])


def _replay_against_eager(warm=2, n=3, **kw):
    """`warm` + `n` eager steps on one twin, GraphedStep(warmup=warm) + `n` replays on the other, learning rates moved between steps."""
    from rot_mvgaze_amd.graph import GraphedStep
    m1, o1, s1 = _setup(**kw)
    start = {k: p.detach().clone() for k, p in m1.named_parameters()}
    buffers = {k: b.detach().clone() for k, b in m1.named_buffers()}
    eager = []
    for _ in range(warm):
        s1()
    for k in range(n):
        _set_lrs(o1, LRS[k])
        eager.append(float(s1().item()))
    m2, o2, s2 = _setup(**kw)
    gs = GraphedStep(m2, s2, o2, warmup=warm)
    graph = []
    for k in range(n):
        _set_lrs(o2, LRS[k])
        graph.append(float(gs.run().item()))
    assert graph == eager, (graph, eager)
    _same_state(m1, o1, m2, o2)
    return m1, o1, m2, o2, start, buffers


@pytest.mark.parametrize("depth,V,B,bf16", [(18, 2, 4, False), (50, 3, 2, False), (50, 2, 2, True)], ids=["r18_fp32", "r50_fp32", "r50_bf16_storage"])
def test_frozen_prefix_and_two_groups_replay_the_eager_step_bit_for_bit(depth, V, B, bf16):
    m1, o1, m2, o2, start, _ = _replay_against_eager(depth=depth, V=V, B=B, bf16=bf16)
    (entry,) = o2.state_dict()["mvg_arena_state"]
    seen = {True: 0, False: 0}
    for (p, off, n), name, steps in zip(m2.grad_arena()[1], _arena_names(m2), entry["steps"]):
        frozen = in_prefix(name)
        seen[frozen] += 1
        assert steps == (0 if frozen else 5), (name, steps)
        if frozen:                                                     # value and both moments untouched
            assert torch.equal(p.detach().view(torch.int32), start[name].view(torch.int32)), name
            assert not entry["exp_avg"][off:off + n].any() and not entry["exp_avg_sq"][off:off + n].any(), name
        else:
            assert not torch.equal(p.detach(), start[name]), name
    assert seen[True] and seen[False]


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_frozen_batchnorm_replays_the_eager_step_bit_for_bit(bf16):
    m1, o1, m2, o2, start, buffers = _replay_against_eager(bf16=bf16, frozen=None, freeze_bn=True)
    for m in (m1, m2):
        checked = 0
        for k, b in m.named_buffers():                                 # the running statistics are what they were
            assert torch.equal(b, buffers[k]), k
            checked += "running_" in k
        assert checked >= 2 * 20                                       # ResNet-18: 20 BatchNorm layers
    steps = _steps(m2, o2)
    assert {steps[k] for k in steps if is_bn_affine(k)} == {0} and {steps[k] for k in steps if not is_bn_affine(k)} == {5}
    for k, p in m2.named_parameters():
        if is_bn_affine(k):
            assert torch.equal(p.detach(), start[k]), k


def test_device_resident_segments_are_the_host_side_segments():
    m1, o1, s1 = _setup(capturable="segments")
    m3, o3, s3 = _setup(capturable=False)
    for _ in range(2):
        s1()
        s3()
        for (k1, p1), (_, p3) in zip(m1.named_parameters(), m3.named_parameters()):
            assert torch.allclose(p1, p3, rtol=2e-6, atol=1e-8), k1
        # (same parameters for the next round: the two flavours only differ in where the scalars come from)
        m3.load_state_dict(m1.state_dict())
    assert _steps(m1, o1) == _steps(m3, o3)


def _unfreeze_layer2(m):
    moved = [k for k, p in m.named_parameters() if in_prefix(k) and ".layer2." in k]
    for k, p in m.named_parameters():
        if k in moved:
            p.requires_grad_(True)
    assert moved
    return moved


def test_plan_change_is_refused_on_replay_and_a_new_capture_continues():
    from rot_mvgaze_amd.graph import GraphedStep
    m2, o2, s2 = _setup()
    gs = GraphedStep(m2, s2, o2, warmup=2)
    gs.run()
    n = 3
    assert set(_steps(m2, o2).values()) == {0, n}
    moved = _unfreeze_layer2(m2)
    arena, (entry,) = m2.param_arena().clone(), o2.state_dict()["mvg_arena_state"]
    with pytest.raises(RuntimeError, match="requires_grad of .* changed.*new GraphedStep"):
        gs.run()
    torch.cuda.synchronize()
    assert torch.equal(m2.param_arena(), arena)                        # nothing was updated
    (after,) = o2.state_dict()["mvg_arena_state"]
    assert after["steps"] == entry["steps"] and torch.equal(after["exp_avg"], entry["exp_avg"])
    # a new capture on the same optimizer continues: its one eager warm-up step replans from the device counters
    gs2 = GraphedStep(m2, s2, o2, warmup=1)
    steps = _steps(m2, o2)
    for k, c in steps.items():
        assert c == (1 if k in moved else 0 if up_to_layer1(k) else n + 1), (k, c)
    gs2.run()
    # the eager twin through the same schedule
    m1, o1, s1 = _setup()
    for _ in range(n):
        s1()
    _unfreeze_layer2(m1)
    s1()
    s1()
    _same_state(m1, o1, m2, o2)
    assert {c for k, c in _steps(m2, o2).items() if k in moved} == {2}
    # ... and betas moved after a capture are refused as well (a by-value constant of the captured plan)
    o2.param_groups[1]["betas"] = (0.8, 0.999)
    with pytest.raises(RuntimeError, match="plan changed.*new GraphedStep"):
        gs2.run()


def test_a_changed_plan_first_seen_inside_a_capture_is_refused():
    m, opt, step = _setup()
    # no eager step yet: the device state does not exist
    step(optimize=False)                                               # gradients, no optimizer step
    torch.cuda.synchronize()
    arena = m.param_arena().clone()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="run one eager step before capturing"):
        with torch.cuda.graph(g):
            opt.step()
    torch.cuda.synchronize()
    assert torch.equal(m.param_arena(), arena)
    # with device state of another plan (betas moved since the eager steps)
    step()
    step()
    opt.param_groups[0]["betas"] = (0.8, 0.99)
    torch.cuda.synchronize()
    arena = m.param_arena().clone()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="run one eager step before capturing"):
        with torch.cuda.graph(g):
            opt.step()
    torch.cuda.synchronize()
    assert torch.equal(m.param_arena(), arena)
    step()                                                             # the eager step replans and goes on
    assert set(_steps(m, opt).values()) == {0, 3}


def test_checkpoint_from_the_device_table_loads_into_the_host_side_optimizer():
    from rot_mvgaze_amd.graph import GraphedStep
    m2, o2, s2 = _setup()
    gs = GraphedStep(m2, s2, o2, warmup=2)
    for k in range(2):
        _set_lrs(o2, LRS[k])
        gs.run()
    sd = o2.state_dict()
    assert set(sd["mvg_arena_state"][0]["steps"]) == {0, 4}
    m3, o3, s3 = _setup(capturable=False)
    m3.load_state_dict(m2.state_dict())
    o3.load_state_dict(sd)
    assert [g["lr"] for g in o3.param_groups] == list(LRS[1])
    s2()                                                               # one eager step each
    s3()
    for (k2, p2), (_, p3) in zip(m2.named_parameters(), m3.named_parameters()):
        assert torch.allclose(p2, p3, rtol=2e-6, atol=1e-8), k2
    assert _steps(m2, o2) == _steps(m3, o3) and set(_steps(m3, o3).values()) == {0, 5}
    # ... and the other way: the host-side checkpoint into a "segments" optimizer
    m4, o4, s4 = _setup()
    m4.load_state_dict(m3.state_dict())
    o4.load_state_dict(o3.state_dict())
    s3()
    s4()
    for (k3, p3), (_, p4) in zip(m3.named_parameters(), m4.named_parameters()):
        assert torch.allclose(p3, p4, rtol=2e-6, atol=1e-8), k3
    assert _steps(m4, o4) == _steps(m3, o3)


def test_one_group_nothing_frozen_goes_through_the_new_entry_point(monkeypatch):
    from rot_mvgaze_amd import ops
    seen = []
    real = ops.adam_step_segments_dev
    monkeypatch.setattr(ops, "adam_step_segments_dev", lambda *a: (seen.append(len(a[4])), real(*a))[1])
    for name in ("adam_step", "adam_step_dev", "adam_step_segments"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name: pytest.fail(f"{_n} ran in capturable='segments' mode"))
    m1, o1, m2, o2, _, _ = _replay_against_eager(frozen=None, groups=False)
    assert set(_steps(m2, o2).values()) == {5}
    assert seen == [1] * (5 + 2 + 1)                                   # one segment: 5 eager steps, 2 warm-up steps, 1 capture
