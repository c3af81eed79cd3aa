"""optim.AdamW and optim.Adam(decoupled_weight_decay=...) on a model (ResNet-18, V = 2, B = 2, 64 x 64 synthetic input; MI355X only).

Eager steps are held per element to the float64 references of tests/adamw_forms_ref.py (decoupled groups) and
tests/adam_forms_ref.py (coupled groups), evaluated from the arenas as they were before the step and the gradient arena - the
units and the bars K_M / K_V / K_P of the kernel-level tests, no new tolerance.  Captured steps (graph.GraphedStep) must replay
the eager steps bit for bit, and a mode flipped after the capture must make run() raise."""
import numpy as np
import pytest
import torch

import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd import synth

import adam_forms_ref as R
import adamw_forms_ref as W

pytestmark = pytest.mark.gpu

BB = "_feat_extractor.0."
_SD = {}


def dev():
    return torch.device("cuda:0")


def in_stem(name):
    return name.startswith(BB) and ".fc." not in name and not any(f".layer{i}." in name for i in (1, 2, 3, 4))


def _setup(make_optimizer, freeze_stem=False):
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    from rot_mvgaze_amd.losses import MultiViewIterationLoss
    from rot_mvgaze_amd.model import MultiViewGaze
    depth, V, B, hw = 18, 2, 2, 64
    if depth not in _SD:
        _SD[depth] = {k: torch.from_numpy(np.array(v)) for k, v in synth.make_state_dict(depth, 0, 3).items()}
    m = MultiViewGaze(depth, 3)
    m.load_state_dict(_SD[depth], strict=True)
    m.to(dev()).train()
    if freeze_stem:
        for k, p in m.named_parameters():
            if in_stem(k):
                p.requires_grad_(False)
    inp = synth.make_inputs(B, V, 77, hw)
    img = [torch.from_numpy(np.ascontiguousarray(inp["img"][:, v])).to(dev()) for v in range(V)]
    gt = torch.from_numpy(inp["gt_gaze"]).to(dev())
    rot = rotation_matrix_2d(torch.from_numpy(inp["head_pose"]).reshape(-1, 2).to(dev())).reshape(B, V, 3, 3)
    crit = MultiViewIterationLoss(rel_weight=0.01, reference_decay=1.0, iter_decay=0.5)
    opt = make_optimizer(m)

    def step(optimize=True):
        m.zero_grad(set_to_none=True)
        loss = crit(m.forward_multiview(img, rot), gt)
        loss.backward()
        if optimize:
            opt.step()
        return loss
    return m, opt, step


def two_groups(m, **kw):
    """Backbone (without the frozen stem) coupled with weight_decay 1e-6, heads decoupled with 1e-2: optim.AdamW's defaults."""
    from rot_mvgaze_amd.optim import AdamW
    head = [p for k, p in m.named_parameters() if not k.startswith("_feat_extractor")]
    bb = [p for k, p in m.named_parameters() if k.startswith("_feat_extractor") and not in_stem(k)]
    return AdamW([{"params": bb, "lr": 1e-4, "decoupled_weight_decay": False, "weight_decay": 1e-6}, {"params": head, "lr": 1e-3}], **kw)


def _entry(opt):
    (entry,) = opt.state_dict()["mvg_arena_state"]
    return entry


def runs_of(entries, ids):
    """[(begin, end)] of the maximal runs of arena-adjacent parameters in ``ids`` that require a gradient, ends on the 4-element
    slot as the planner rounds them (the padding holds zeros and maps to zeros)."""
    out = []
    for p, off, cnt in entries:
        if id(p) not in ids or not p.requires_grad:
            continue
        end = (off + cnt + 3) // 4 * 4
        if out and out[-1][1] == off:
            out[-1][1] = end
        else:
            out.append([off, end])
    return [tuple(r) for r in out]


def held_step(m, opt, step, number, label):
    """Step ``number`` of a fresh run, eager: the steps before it unheld, then backward, the arenas as they are, opt.step(), every
    group's elements against its own reference and everything else bit for bit."""
    for _ in range(number - 1):
        step()
    step(optimize=False)
    arena_g, entries = m.grad_arena()
    n = m.param_arena().numel()
    p0, g = m.param_arena().detach().cpu().numpy().copy(), arena_g.detach().cpu().numpy().copy()
    if number == 1:
        m0, v0 = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    else:
        e = _entry(opt)
        m0, v0 = e["exp_avg"].cpu().numpy(), e["exp_avg_sq"].cpu().numpy()
    opt.step()
    torch.cuda.synchronize()
    e = _entry(opt)
    p1, m1, v1 = m.param_arena().detach().cpu().numpy(), e["exp_avg"].cpu().numpy(), e["exp_avg_sq"].cpu().numpy()
    touched = np.zeros(n, dtype=bool)
    for gi, group in enumerate(opt.param_groups):
        decoupled = group["decoupled_weight_decay"]
        ref = W.reference if decoupled else R.reference
        K = (W.K_M, W.K_V, W.K_P) if decoupled else (R.K_M, R.K_V, R.K_P)
        runs = runs_of(entries, {id(p) for p in group["params"]})
        w, rel, moved = [0.0, 0.0, 0.0], 0.0, 0.0
        for b, e_ in runs:
            touched[b:e_] = True
            r = ref(p0[b:e_], g[b:e_], m0[b:e_], v0[b:e_], group["lr"], group["betas"][0], group["betas"][1], group["eps"],
                    group["weight_decay"], number)
            x = R.worst_units(r, p1[b:e_], m1[b:e_], v1[b:e_])
            w = [a if (a != a or a >= c) else c for a, c in zip(x, w)]
            rel, moved = max(rel, W.step_max_rel(r, p0[b:e_], p1[b:e_])), max(moved, float(np.abs(r["d"]).max()))
        print(f"ADAMW-OPTIM {label} step {number} group {gi} ({'decoupled' if decoupled else 'coupled'}, wd {group['weight_decay']:g}, "
              f"{sum(e_ - b for b, e_ in runs)} elements in {len(runs)} run(s)): m {w[0]:.3f} v {w[1]:.3f} p {w[2]:.3f}   step max-rel {rel:.3e}")
        assert all(np.isfinite(x) for x in w) and w[0] <= K[0] and w[1] <= K[1] and w[2] <= K[2], (label, number, gi, w, K)
        assert moved > 0, "the group received a gradient and moved"
    # frozen and group-less parameters: value and both moments bit for bit
    rest = ~touched
    for got, old, what in zip((p1, m1, v1), (p0, m0, v0), ("param", "exp_avg", "exp_avg_sq")):
        changed = np.flatnonzero((got.view(np.int32) != old.view(np.int32)) & rest)
        assert changed.size == 0, f"{label} step {number}: {what} changed at {changed[:5].tolist()} outside every group's parameters"
    in_group = {id(p) for group in opt.param_groups for p in group["params"]}
    assert e["steps"] == [number if p.requires_grad and id(p) in in_group else 0 for (p, _, _) in entries]
    return int(rest.sum())


@pytest.mark.parametrize("number", [1, 2, 3])
def test_three_eager_adamw_steps_follow_the_decoupled_reference(number):
    from rot_mvgaze_amd.optim import AdamW
    m, opt, step = _setup(lambda m: AdamW(m.parameters(), lr=1e-3))
    assert opt.param_groups[0]["weight_decay"] == 1e-2 and opt.param_groups[0]["decoupled_weight_decay"] is True
    held_step(m, opt, step, number, "AdamW one group")


@pytest.mark.parametrize("number", [1, 2])
def test_two_groups_with_a_frozen_stem_each_follow_their_own_reference(number):
    m, opt, step = _setup(two_groups, freeze_stem=True)
    assert [g["decoupled_weight_decay"] for g in opt.param_groups] == [False, True]
    stem = [p for k, p in m.named_parameters() if in_stem(k)]
    assert stem and not any(p.requires_grad for p in stem)
    untouched = held_step(m, opt, step, number, "backbone coupled + heads decoupled, stem frozen")
    assert untouched >= sum(p.numel() for p in stem)


def _same_state(m1, o1, m2, o2):
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    for k in sd1:
        assert torch.equal(sd1[k], sd2[k]), k
    e1, e2 = _entry(o1), _entry(o2)
    assert e1["steps"] == e2["steps"]
    assert torch.equal(e1["exp_avg"], e2["exp_avg"]) and torch.equal(e1["exp_avg_sq"], e2["exp_avg_sq"])
    assert bool(e1["exp_avg"].any())


def _eager_against_replays(make_optimizer, freeze_stem, lrs):
    from rot_mvgaze_amd.graph import GraphedStep
    m1, o1, s1 = _setup(make_optimizer, freeze_stem)
    for _ in range(2):
        s1()
    for lr in lrs:
        o1.param_groups[-1]["lr"] = lr               # a scheduler stepping between iterations
        s1()
    m2, o2, s2 = _setup(make_optimizer, freeze_stem)
    gs = GraphedStep(m2, s2, o2, warmup=2)
    for lr in lrs:
        o2.param_groups[-1]["lr"] = lr
        gs.run()
    torch.cuda.synchronize()
    _same_state(m1, o1, m2, o2)
    assert max(_entry(o2)["steps"]) == 2 + len(lrs)
    return m2, o2, gs


def test_captured_segmented_adamw_with_clipping_replays_the_eager_steps_and_refuses_a_flipped_mode():
    make = lambda m: two_groups(m, capturable="segments", max_grad_norm=1.0, skip_nonfinite=True)
    m2, o2, gs = _eager_against_replays(make, True, [1e-3, 5e-4, 2e-3])
    (rep,) = o2.grad_clip_report()
    assert not rep["skipped"] and rep["skipped_total"] == 0 and rep["norm"] > 0
    # the mode travels by value in the captured launches: a flip must not replay
    o2.param_groups[0]["decoupled_weight_decay"] = True
    with pytest.raises(RuntimeError, match="plan changed since the capture"):
        gs.run()
    o2.param_groups[0]["decoupled_weight_decay"] = False
    gs.run()                                                                         # ... and flipped back it does again


def test_captured_adamw_with_one_group_replays_the_eager_steps():
    from rot_mvgaze_amd.optim import AdamW
    _eager_against_replays(lambda m: AdamW(m.parameters(), lr=1e-3, capturable=True), False, [1e-3, 5e-4, 2e-3])
