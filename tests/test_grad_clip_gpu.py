"""Global-norm gradient clipping and the non-finite guard of the segmented Adam steps, at kernel level and through optim.Adam.

Bars.  The device record {norm, coef, skipped, skipped_total} against the float64 reference of tests/grad_clip_ref.py rounded to
float32: within ONE float32 ulp - the kernel's double sum over <= 1e8 exact squares is good to 1e-8 relative at the very worst, far
inside a float32 ulp (6e-8 .. 1.2e-7), so after sqrt and the division the two doubles can round to different floats only across
one rounding boundary.  The clipped updates against the EXISTING ops.adam_step_segments / adam_step_segments_dev on clones whose
gradient torch first multiplied by the recorded coefficient in fp32 (g.mul(coef)): torch.equal on parameters, both moments and the
state rows - the clipped kernels round the product to fp32 on its own and then run the same adam_elem.  Everything outside the
segments: unchanged as int32.  Kernel-level arenas, segment shapes and RNG are those of tests/test_adam_segments_dev_gpu.py."""
import numpy as np
import pytest
import torch

import grad_clip_ref as ref
import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd import _lib, ops, synth

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


# ================================================================ kernel level
def _arena(n, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g).to(dev())
    gr = (torch.randn(n, generator=g) * 0.1).to(dev())
    m = (torch.randn(n, generator=g) * 0.01).to(dev())
    v = (torch.rand(n, generator=g) * 1e-3).to(dev())
    return p, gr, m, v


def _rows(counts):
    return torch.tensor([[float(c), 0.0, 0.0] for c in counts], dtype=torch.float32).reshape(-1, 3).to(dev())


THREE = [(0, 4, 1, 0.9, 0.999, 1e-8, 0.0),                    # a 4-element segment starting at 0
         (64, 1028, 0, 0.8, 0.99, 1e-6, 1e-6),                # ... a hole before and behind this one
         (2048, 4096, 1, 0.5, 0.9, 1e-3, 1e-2)]               # ... and one ending at n; it shares lr entry 1 with the first
THREE_COUNTS, THREE_LRS = [0, 4, 99], [1e-4, 5e-2]
LRS5 = [1e-5, 1e-4, 1e-3, 3e-3, 1e-2]


def _random_segments(seed=3):
    rng = np.random.default_rng(seed)
    segs, counts, off = [], [], 0
    for i in range(35):                                                              # 16 + 16 + 3: three chunk launches
        off += 4 * int(rng.integers(0, 5))                                           # holes of 0 .. 16 elements
        ln = 4 * int(rng.integers(1, 17))                                            # 4 .. 64 elements
        segs.append((off, off + ln, int(rng.integers(0, 5)), float(rng.uniform(0.5, 0.95)), float(rng.uniform(0.9, 0.9999)), 1e-8,
                     float(rng.choice([0.0, 1e-6, 1e-2]))))
        counts.append(int(rng.integers(0, 50)))
        off += ln
    assert len(segs) == 35
    return segs, counts, off + 64


def _cases():
    segs, counts, n = _random_segments()
    return {"three": (4096, THREE, THREE_COUNTS, THREE_LRS), "thirty_five": (n, segs, counts, LRS5)}


CASES = _cases()


def _bounds(segs):
    return [(s[0], s[1]) for s in segs]


def _outside(n, segs):
    mask = torch.ones(n, dtype=torch.bool, device=dev())
    for b, e, *_ in segs:
        mask[b:e] = False
    return mask


def _host_form(segs, lrs, counts, call):
    """The (begin, end, lr, b1, b2, eps, wd, step) records of ops.adam_step_segments for the `call`-th step (0-based)."""
    return [(b, e, lrs[li], b1, b2, eps, wd, c + 1 + call) for (b, e, li, b1, b2, eps, wd), c in zip(segs, counts)]


def _record(clip4):
    return clip4.cpu().numpy().copy()


def _check_record(rec, grad, bounds, max_norm, skip=False):
    r = ref.reference(grad, bounds, max_norm, skip)
    want_norm, want_coef = ref.record(r)
    assert ref.within_one_ulp(rec[0], want_norm), f"norm {rec[0]!r} vs {want_norm!r}"
    assert ref.within_one_ulp(rec[1], want_coef), f"coef {rec[1]!r} vs {want_coef!r}"
    assert rec[2] == (1.0 if r["skipped"] else 0.0)
    return r


# ---------------------------------------------------------------- the norm
@pytest.mark.parametrize("poison", [float("nan"), 1e30], ids=["nan_outside", "1e30_outside"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_norm_reads_the_segments_only_and_repeats_bit_for_bit(case, poison):
    n, segs, _, _ = CASES[case]
    g = _arena(n, 0)[1]
    g[_outside(n, segs)] = poison                                                    # every element outside the segments
    for max_norm in (0.5, 1e9, None):
        clip4 = torch.zeros(4, device=dev())
        ops.grad_norm_segments(g, _bounds(segs), max_norm, True, clip4)
        first = _record(clip4)
        r = _check_record(first, g, _bounds(segs), max_norm, skip=True)
        assert first[2] == 0.0 and first[3] == 0.0 and np.isfinite(first[0])
        assert (first[1] < 1.0) == (max_norm == 0.5) and (max_norm == 0.5 or first[1] == 1.0) and not r["skipped"]
        ops.grad_norm_segments(g, _bounds(segs), max_norm, True, clip4)
        assert _record(clip4).view(np.int32).tolist() == first.view(np.int32).tolist()


def test_double_accumulation_survives_one_huge_element():
    """1e20^2 = 1e40 overflows a float accumulator (the norm would be inf); the double one holds it."""
    n, segs = 4096, THREE
    g = _arena(n, 1)[1] * 10.0
    g[500] = 1e20
    clip4 = torch.zeros(4, device=dev())
    ops.grad_norm_segments(g, _bounds(segs), 1.0, True, clip4)
    rec = _record(clip4)
    _check_record(rec, g, _bounds(segs), 1.0, skip=True)
    assert np.isfinite(rec[0]) and rec[0] >= 1e20 and rec[2] == 0.0 and 0.0 < rec[1] < 1e-19


def test_grid_stride_loop():
    cap = _lib.lib().mvg_grad_norm_workspace_bytes(1) // 8                           # workgroups of one chunk launch, at most
    assert cap >= 1
    ln = 1 << 22
    while cap * 256 * 4 >= ln:                                                       # more than one pass of the loop
        ln *= 2
    segs = [(1024, 1024 + ln)]
    g = (torch.randn(ln + 4096, generator=torch.Generator().manual_seed(2)) * 0.1).to(dev())
    g[:1024] = float("nan")
    g[1024 + ln:] = float("nan")
    clip4 = torch.zeros(4, device=dev())
    ops.grad_norm_segments(g, segs, 1.0, True, clip4)
    _check_record(_record(clip4), g, segs, 1.0, skip=True)


# ---------------------------------------------------------------- the clipped updates
def _run_host(p, g, m, v, segs, lrs, counts, calls, clip=None):
    """`calls` steps of the host-side segmented form; clip = (max_norm, skip, clip4): the norm in front of each clipped step."""
    for call in range(calls):
        if clip is None:
            ops.adam_step_segments(p, g, m, v, _host_form(segs, lrs, counts, call))
        else:
            ops.grad_norm_segments(g, _bounds(segs), clip[0], clip[1], clip[2])
            ops.adam_step_segments_clip(p, g, m, v, _host_form(segs, lrs, counts, call), clip[2])


def _run_dev(p, g, m, v, segs, lr_dev, state, calls, clip=None):
    for _ in range(calls):
        if clip is None:
            ops.adam_step_segments_dev(p, g, m, v, segs, lr_dev, state)
        else:
            ops.grad_norm_segments(g, _bounds(segs), clip[0], clip[1], clip[2])
            ops.adam_step_segments_dev_clip(p, g, m, v, segs, lr_dev, state, clip[2])


def _clipped_against_scaled(case, form, max_norm, calls=2):
    """Returns (clipped, reference on the torch-scaled gradient, unclipped) arenas [p, m, v(, state)] and the record."""
    n, segs, counts, lrs = CASES[case]
    runs = []
    clip4 = torch.zeros(4, device=dev())
    g = _arena(n, 0)[1]
    ops.grad_norm_segments(g, _bounds(segs), max_norm, False, clip4)                # the coefficient both calls will see
    coef = float(clip4[1].item())
    for which in ("clipped", "scaled", "unclipped"):
        p, g, m, v = _arena(n, 0)
        grad = g.mul(coef) if which == "scaled" else g                               # torch, fp32
        clip = (max_norm, False, clip4) if which == "clipped" else None
        if form == "host":
            _run_host(p, grad, m, v, segs, lrs, counts, calls, clip)
            runs.append([p, m, v])
        else:
            lr_dev, state = torch.tensor(lrs, dtype=torch.float32).to(dev()), _rows(counts)
            _run_dev(p, grad, m, v, segs, lr_dev, state, calls, clip)
            runs.append([p, m, v, state])
        if which == "clipped":
            assert torch.equal(grad, _arena(n, 0)[1])                                # the gradient arena is not rewritten
    torch.cuda.synchronize()
    return runs, _record(clip4), (n, segs, counts)


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_clipped_update_is_the_existing_step_on_a_torch_scaled_gradient(case, form):
    (clipped, scaled, unclipped), rec, (n, segs, counts) = _clipped_against_scaled(case, form, max_norm=0.05)
    assert 0.0 < rec[1] < 0.5 and rec[2] == 0.0                                      # the clip binds
    for got, want, what in zip(clipped, scaled, ("param", "exp_avg", "exp_avg_sq", "state rows")):
        assert torch.equal(got, want), what
    # the moments scale with coef and coef^2 (Adam's parameter update is nearly scale-invariant and would hide a missing multiply)
    for b, e, *_ in segs:
        assert not torch.equal(clipped[1][b:e], unclipped[1][b:e]) and not torch.equal(clipped[2][b:e], unclipped[2][b:e])
    before = [_arena(n, 0)[i] for i in (0, 2, 3)]
    out = _outside(n, segs)
    for got, old, what in zip(clipped, before, ("param", "exp_avg", "exp_avg_sq")):
        assert torch.equal(got[out].view(torch.int32), old[out].view(torch.int32)), f"{what} outside the segments"
    if form == "dev":
        assert clipped[3][:, 0].tolist() == [float(c + 2) for c in counts]


@pytest.mark.parametrize("form", ["host", "dev"])
def test_a_clip_that_does_not_bind_is_the_unclipped_step(form):
    (clipped, scaled, unclipped), rec, _ = _clipped_against_scaled("three", form, max_norm=1e9)
    assert rec[1] == 1.0
    for got, want in zip(clipped, unclipped):
        assert torch.equal(got, want)


# ---------------------------------------------------------------- the guard
@pytest.mark.parametrize("case", sorted(CASES))
def test_guard_skips_a_nonfinite_step_and_the_next_clean_one_is_as_if_it_never_happened(case):
    n, segs, counts, lrs = CASES[case]
    clean = _arena(n, 0)[1]
    for form in ("host", "dev"):
        p, g, m, v = _arena(n, 0)
        lr_dev, state = torch.tensor(lrs, dtype=torch.float32).to(dev()), _rows(counts)
        before = [t.clone() for t in (p, m, v, state)]
        clip4 = torch.zeros(4, device=dev())
        where = segs[len(segs) // 2][0] + 1                                          # inside a segment of the second chunk (35) / the middle one
        for k, bad in enumerate((float("nan"), float("inf"))):
            g.copy_(clean)
            g[where] = bad
            if form == "host":
                _run_host(p, g, m, v, segs, lrs, counts, 1, (0.05, True, clip4))
            else:
                _run_dev(p, g, m, v, segs, lr_dev, state, 1, (0.05, True, clip4))
            rec = _record(clip4)
            assert rec[2] == 1.0 and rec[1] == 0.0 and rec[3] == k + 1 and not np.isfinite(rec[0])
            for got, old, what in zip((p, m, v, state), before, ("param", "exp_avg", "exp_avg_sq", "state rows")):
                assert torch.equal(got.view(torch.int32), old.view(torch.int32)), f"{what} after a skipped step ({bad})"
        # a clean call: what a fresh arena gives in its first step
        g.copy_(clean)
        p2, g2, m2, v2 = _arena(n, 0)
        state2, clip2 = _rows(counts), torch.zeros(4, device=dev())
        if form == "host":
            _run_host(p, g, m, v, segs, lrs, counts, 1, (0.05, True, clip4))
            _run_host(p2, g2, m2, v2, segs, lrs, counts, 1, (0.05, True, clip2))
        else:
            _run_dev(p, g, m, v, segs, lr_dev, state, 1, (0.05, True, clip4))
            _run_dev(p2, g2, m2, v2, segs, lr_dev, state2, 1, (0.05, True, clip2))
            assert state[:, 0].tolist() == [float(c + 1) for c in counts]            # advanced once
        for got, want in zip((p, m, v, state), (p2, m2, v2, state2)):
            assert torch.equal(got, want)
        assert not torch.equal(p, before[0])
        rec = _record(clip4)
        assert rec[2] == 0.0 and rec[3] == 2.0 and _record(clip2)[:3].tolist() == rec[:3].tolist()


def test_a_nan_in_a_hole_does_not_skip():
    n, segs = 4096, THREE
    g = _arena(n, 0)[1]
    g[32] = float("nan")                                                             # between the first and the second segment
    clip4 = torch.zeros(4, device=dev())
    ops.grad_norm_segments(g, _bounds(segs), 0.05, True, clip4)
    rec = _record(clip4)
    assert rec[2] == 0.0 and rec[3] == 0.0 and np.isfinite(rec[0]) and 0.0 < rec[1] < 1.0


def test_without_the_guard_a_nan_gradient_turns_the_slices_nan_as_torch_does():
    """Pins the documented behaviour: skip_nonfinite=False is clip_grad_norm_(error_if_nonfinite=False) - the coefficient is NaN,
    every scaled gradient is NaN, and the update carries it into the segments (and nowhere else)."""
    n, segs, counts, lrs = CASES["three"]
    p, g, m, v = _arena(n, 0)
    before = [t.clone() for t in (p, m, v)]
    g[100] = float("nan")
    clip4 = torch.zeros(4, device=dev())
    _run_host(p, g, m, v, segs, lrs, counts, 1, (0.05, False, clip4))
    rec = _record(clip4)
    assert np.isnan(rec[0]) and np.isnan(rec[1]) and rec[2] == 0.0 and rec[3] == 0.0
    for b, e, *_ in segs:
        assert bool(torch.isnan(p[b:e]).all()) and bool(torch.isnan(m[b:e]).all())
    out = _outside(n, segs)
    for got, old in zip((p, m, v), before):
        assert torch.equal(got[out].view(torch.int32), old[out].view(torch.int32))


# ---------------------------------------------------------------- rejections
SENTINEL = [7.0, 0.25, 0.0, 3.0]


@pytest.mark.parametrize("what,match", [("short_ws", "workspace"), ("null_clip4", "null"), ("unsorted", "unsorted"),
                                        ("unaligned", "aligned")])
def test_bad_norm_calls_are_rejected_before_any_launch(what, match):
    n = 4096
    g = _arena(n, 2)[1]
    clip4 = torch.tensor(SENTINEL, device=dev())
    bounds = {"unsorted": [(64, 128), (0, 32)], "unaligned": [(0, 64), (130, 194)]}.get(what, [(0, 64), (128, 256)])
    ws = None
    if what == "short_ws":
        bounds = [(0, 2048)]                                                         # two workgroups: 16 bytes of partials
        ws = torch.empty(8, dtype=torch.uint8, device=dev())                         # ... and room for one
    with pytest.raises(RuntimeError, match="grad_norm_segments: .*" + match):
        ops.grad_norm_segments(g, bounds, 1.0, True, None if what == "null_clip4" else clip4, ws)
    torch.cuda.synchronize()
    assert clip4.tolist() == SENTINEL


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("what,match", [("null_clip4", "null clip4"), ("unsorted", "unsorted"), ("unaligned", "aligned")])
def test_bad_clipped_steps_are_rejected_before_any_launch(form, what, match):
    n = 4096
    p, g, m, v = _arena(n, 2)
    bounds = {"unsorted": [(64, 128), (0, 32)], "unaligned": [(0, 64), (130, 194)]}.get(what, [(0, 64), (128, 256)])
    clip4 = None if what == "null_clip4" else torch.tensor([1.0, 0.5, 0.0, 0.0], device=dev())
    state = _rows([3, 3])
    before = [t.clone() for t in (p, m, v, state)]
    with pytest.raises(RuntimeError, match="adam_step_segments_(dev_)?clip: .*" + match):
        if form == "host":
            ops.adam_step_segments_clip(p, g, m, v, [(b, e, 1e-3, 0.9, 0.999, 1e-8, 0.0, 4) for b, e in bounds], clip4)
        else:
            ops.adam_step_segments_dev_clip(p, g, m, v, [(b, e, 0, 0.9, 0.999, 1e-8, 0.0) for b, e in bounds],
                                            torch.tensor([1e-3], device=dev()), state, clip4)
    torch.cuda.synchronize()
    for got, old in zip((p, m, v, state), before):                                   # neither the valid first segment nor the tick ran
        assert torch.equal(got.view(torch.int32), old.view(torch.int32))


# ================================================================ model level
# ResNet-18, V=2, B=3, 64 px (the b3_hw64 shape of the fixtures); the stem and layer1 frozen and in no group, two parameter groups
# (head; layer2-4 of the backbone).
# The non-finite step: the loss is multiplied by a static device scalar (1 in a clean step, NaN in the bad one), so the upstream
# gradient - and with it every gradient of the step - is NaN while the forward, and BatchNorm's running statistics with it, stay
# clean.  NaN LABELS cannot serve here: the angular loss kernel takes its gradient only where -1 < cos < 1, which a NaN cosine
# fails, so a NaN in gt_gaze gives a ZERO gradient (and a loss of 180 degrees), not a non-finite one.
BB = "_feat_extractor.0."
_SD, _PROBE = {}, {}


def frozen(name):
    return name.startswith(BB) and ".fc." not in name and not any(f".layer{i}." in name for i in (2, 3, 4))


def _setup(capturable=False, **clip):
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    from rot_mvgaze_amd.losses import MultiViewIterationLoss
    from rot_mvgaze_amd.model import MultiViewGaze
    from rot_mvgaze_amd.optim import Adam
    depth, V, B, hw = 18, 2, 3, 64
    if depth not in _SD:
        _SD[depth] = {k: torch.from_numpy(np.array(v)) for k, v in synth.make_state_dict(depth, 0, 3).items()}
    m = MultiViewGaze(depth, 3)
    m.load_state_dict(_SD[depth], strict=True)
    m.to(dev()).train()
    for k, p in m.named_parameters():
        if frozen(k):
            p.requires_grad_(False)
    inp = synth.make_inputs(B, V, 77, hw)
    img = [torch.from_numpy(np.ascontiguousarray(inp["img"][:, v])).to(dev()) for v in range(V)]
    gt = torch.from_numpy(inp["gt_gaze"]).to(dev())
    rot = rotation_matrix_2d(torch.from_numpy(inp["head_pose"]).reshape(-1, 2).to(dev())).reshape(B, V, 3, 3)
    crit = MultiViewIterationLoss(rel_weight=0.01, reference_decay=1.0, iter_decay=0.5)
    head = [p for k, p in m.named_parameters() if not k.startswith("_feat_extractor")]
    bb = [p for k, p in m.named_parameters() if k.startswith("_feat_extractor") and not frozen(k)]
    opt = Adam([{"params": head, "lr": 1e-3, "weight_decay": 0.0}, {"params": bb, "lr": 1e-4, "weight_decay": 1e-6}], capturable=capturable,
               **clip)

    scale = torch.ones((), device=dev())

    def step(optimize=True):
        m.zero_grad(set_to_none=True)
        loss = crit(m.forward_multiview(img, rot), gt) * scale
        loss.backward()
        if optimize:
            opt.step()
        return loss
    return m, opt, step, scale


def _probe_norm():
    """The gradient norm of the first step, from an unclipped probe (guard only: coef stays 1)."""
    if "norm" not in _PROBE:
        m, opt, step, _ = _setup(skip_nonfinite=True)
        step()
        (rep,) = opt.grad_clip_report()
        assert rep["coef"] == 1.0 and not rep["skipped"] and rep["skipped_total"] == 0 and rep["norm"] > 0
        _PROBE["norm"] = rep["norm"]
    return _PROBE["norm"]


def _participating(m):
    """[(begin, end)] of the parameters that hold a gradient written by backward, from the arena layout."""
    return [(off, off + n) for (p, off, n) in m.grad_arena()[1] if p.requires_grad]


def _entry(opt):
    (entry,) = opt.state_dict()["mvg_arena_state"]
    return entry


def _same_state(m1, o1, m2, o2):
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    for k in sd1:
        assert torch.equal(sd1[k], sd2[k]), k
    e1, e2 = _entry(o1), _entry(o2)
    assert e1["steps"] == e2["steps"]
    assert torch.equal(e1["exp_avg"], e2["exp_avg"]) and torch.equal(e1["exp_avg_sq"], e2["exp_avg_sq"])


def test_eager_clipped_step_against_a_twin_with_a_scaled_gradient_arena():
    max_norm = 0.5 * _probe_norm()
    m, opt, step, _ = _setup(max_grad_norm=max_norm)
    step(optimize=False)
    stale = next(p for k, p in m.named_parameters() if frozen(k))
    stale.grad = torch.full_like(stale, 1e6)                                         # a frozen parameter's stale gradient: not in the norm
    arena_g = m.grad_arena()[0]
    unscaled = arena_g.clone()
    want = ref.reference(arena_g, _participating(m), max_norm, False)
    opt.step()
    rec = opt.clip_record(m).cpu().numpy()
    (rep,) = opt.grad_clip_report()
    assert rep["norm"] == float(rec[0]) and rep["coef"] == float(rec[1]) and not rep["skipped"]
    want_norm, want_coef = ref.record(want)
    assert ref.within_one_ulp(rec[0], want_norm) and ref.within_one_ulp(rec[1], want_coef), (rec, want)
    assert rec[0] < 1e5 and 0.4 < rec[1] < 0.6                                       # (half the probe's norm; 1e6 was not seen)
    assert torch.equal(m.grad_arena()[0], unscaled)                                  # .grad keeps the unscaled gradient
    # the twin: the unclipped optimizer on a gradient arena scaled in place by the recorded coefficient
    m2, opt2, step2, _ = _setup()
    step2(optimize=False)
    for b, e in _participating(m2):
        assert torch.equal(m2.grad_arena()[0][b:e], unscaled[b:e])
    m2.grad_arena()[0].mul_(float(rec[1]))
    opt2.step()
    e1, e2 = _entry(opt), _entry(opt2)
    assert torch.equal(e1["exp_avg"], e2["exp_avg"]) and torch.equal(e1["exp_avg_sq"], e2["exp_avg_sq"])
    assert torch.equal(m.param_arena(), m2.param_arena()) and e1["steps"] == e2["steps"]
    assert bool(e1["exp_avg"].any())


def test_captured_step_clips_skips_and_refuses_a_changed_max_grad_norm():
    from rot_mvgaze_amd.graph import GraphedStep
    max_norm = 0.5 * _probe_norm()
    kw = dict(capturable="segments", max_grad_norm=max_norm, skip_nonfinite=True)
    m1, o1, s1, scale1 = _setup(**kw)
    for _ in range(2 + 3):
        s1()
    m2, o2, s2, scale2 = _setup(**kw)
    gs = GraphedStep(m2, s2, o2, warmup=2)
    for _ in range(3):
        gs.run()
    _same_state(m1, o1, m2, o2)
    (rep,) = o2.grad_clip_report()
    assert rep["coef"] < 1.0 and not rep["skipped"] and rep["skipped_total"] == 0
    assert o1.grad_clip_report() == [rep]
    # one replay with a NaN upstream gradient (the forward stays clean: BatchNorm's running statistics must): nothing moves, no
    # row advances
    arena, entry = m2.param_arena().clone(), _entry(o2)
    scale2.fill_(float("nan"))
    gs.run()
    torch.cuda.synchronize()
    after = _entry(o2)
    assert torch.equal(m2.param_arena().view(torch.int32), arena.view(torch.int32))
    assert torch.equal(after["exp_avg"].view(torch.int32), entry["exp_avg"].view(torch.int32))
    assert torch.equal(after["exp_avg_sq"].view(torch.int32), entry["exp_avg_sq"].view(torch.int32))
    assert after["steps"] == entry["steps"] and max(after["steps"]) == 5
    (rep,) = o2.grad_clip_report()
    assert rep["skipped"] and rep["skipped_total"] == 1 and rep["coef"] == 0.0
    # the next clean replay is the twin's next step (the twin ran the skipped step too: its forward moves the running statistics)
    scale2.fill_(1.0)
    gs.run()
    scale1.fill_(float("nan"))
    s1()
    scale1.fill_(1.0)
    s1()
    _same_state(m1, o1, m2, o2)
    assert max(_entry(o2)["steps"]) == 6 and o2.grad_clip_report()[0]["skipped_total"] == 1
    # max_grad_norm travels by value in the captured launches
    o2.max_grad_norm = 2.0 * max_norm
    with pytest.raises(RuntimeError, match="no longer matches"):
        gs.run()


def test_host_side_guard_leaves_the_step_counts_alone():
    m, opt, step, scale = _setup(skip_nonfinite=True, max_grad_norm=0.5 * _probe_norm())
    step()
    entry, arena = _entry(opt), m.param_arena().clone()
    assert set(entry["steps"]) == {0, 1}
    scale.fill_(float("nan"))
    step()
    after = _entry(opt)
    assert after["steps"] == entry["steps"] and after["step"] == entry["step"] == 1
    assert opt.state_dict()["mvg_arena_state"][0]["steps"] == entry["steps"]
    assert torch.equal(m.param_arena().view(torch.int32), arena.view(torch.int32))
    assert torch.equal(after["exp_avg"].view(torch.int32), entry["exp_avg"].view(torch.int32))
    (rep,) = opt.grad_clip_report()
    assert rep["skipped"] and rep["skipped_total"] == 1
