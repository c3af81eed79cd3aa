"""The inference session on the GPU: one mvg_session_forward call against the Python module.

Every comparison is torch.equal on all four outputs (img_feat, lifted, feats, preds): the session queues the same entry
points with the same arguments, so there is no tolerance.  The reference is the same model in eval() under torch.no_grad()
through run_views, on the same inputs.

The 2 GiB guard of the split path is evaluated by the session from the cfg's real sizes (Backbone._guard_scale is a test
hook of the Python module only): test_guard_is_evaluated_from_the_real_sizes compares with the guard not tripped, and checks
on the host plan that a shape which does trip it leaves the split kernels.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd import synth

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


_MODELS = {}


def _model(depth, **variant):
    """One eval-mode model per (depth, variant) for the whole file; tests that change weights build their own (fresh=True)."""
    from rot_mvgaze_amd.arch import Variant
    from rot_mvgaze_amd.model import FeatRotationSymm
    fresh = variant.pop("fresh", False)
    key = (depth, tuple(sorted(variant.items())))
    if fresh or key not in _MODELS:
        sd = synth.make_state_dict(depth, 0, 3, perturb_bn=True, variant=Variant(**variant))
        m = FeatRotationSymm(depth, 3, **variant)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
        m.to(dev()).eval()
        m.ensure_layout()
        if fresh:
            return m
        _MODELS[key] = m
    return _MODELS[key]


def _inputs(B, V, hw, seed=1234):
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    inp = synth.make_inputs(B, V, seed, hw)
    img, hp = torch.from_numpy(inp["img"]), torch.from_numpy(inp["head_pose"])
    imgs = [img[:, v].contiguous().to(dev()) for v in range(V)]
    rot = torch.stack([rotation_matrix_2d(hp[:, v].contiguous().to(dev())) for v in range(V)], dim=1).contiguous()
    return imgs, rot


def _python(m, imgs, rot):
    with torch.no_grad():
        out = m.run_views(imgs, rot)
    return [o.detach().clone() for o in out]


def _same(got, want):
    names = ("img_feat", "lifted", "feats", "preds")
    assert len(got) == len(want) == 4
    for n, a, b in zip(names, got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, n
        assert torch.isfinite(b).all(), n
        assert torch.equal(a, b), f"{n}: max |diff| {(a - b).abs().max().item():.3e}"


def _session(m, V, B, hw, **kw):
    from rot_mvgaze_amd.session import InferenceSession
    return InferenceSession(m, V, B, hw, hw, **kw)


def _check(depth, V, B, hw, **variant):
    m = _model(depth, **variant)
    imgs, rot = _inputs(B, V, hw)
    want = _python(m, imgs, rot)
    with _session(m, V, B, hw) as s:
        _same(s.run(imgs, rot), want)
        return s.launches


# ---------------------------------------------------------------- 1. the batched BatchNorm fold
def _fold_batch(cs, seed=0):
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import check, lib
    g = torch.Generator().manual_seed(seed)
    recs, tensors, outs = [], [], []
    for c in cs:
        gamma, beta = (torch.rand(c, generator=g) + 0.5).to(dev()), (torch.rand(c, generator=g) - 0.5).to(dev())
        rm, rv = (torch.rand(c, generator=g) - 0.5).to(dev()), (torch.rand(c, generator=g) * 2 + 1e-3).to(dev())
        out = torch.full((2, c), float("nan"), device=dev())
        tensors.append((gamma, beta, rm, rv))
        outs.append(out)
        recs.append((gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), c, 0))
    items = np.array(recs, dtype=np.dtype([("g", "<i8"), ("b", "<i8"), ("m", "<i8"), ("v", "<i8"), ("sc", "<i8"), ("sh", "<i8"),
                                           ("c", "<i4"), ("pad", "<i4")]))
    assert items.itemsize == 56
    table = torch.from_numpy(items.view(np.uint8).copy()).to(dev())
    check(lib().mvg_bn_eval_affine_batch(C.c_void_p(table.data_ptr()), len(cs), max(cs), 1e-5, C.c_void_p(ops._s())), "bn_eval_affine_batch")
    for (gamma, beta, rm, rv), out, c in zip(tensors, outs, cs):
        ref = torch.empty(2, 1, c, device=dev())
        ops.bn_eval_affine(1, c, gamma, beta, rm, rv, 1e-5, ref[0], ref[1])
        assert torch.equal(out.view(torch.int32), ref.view(2, c).view(torch.int32)), c


@pytest.mark.parametrize("cs", [[64], [256], [2048], [64, 2048, 256, 128, 512, 64, 1024]])
def test_bn_eval_affine_batch_matches_the_per_unit_fold(cs):
    _fold_batch(cs)


# ---------------------------------------------------------------- 2. split path, small heads
@pytest.mark.parametrize("depth,V,B,hw", [(18, 2, 3, 64), (50, 2, 2, 64), (50, 3, 1, 96), (50, 2, 1, 224)])
def test_split_path_matches_python(depth, V, B, hw):
    assert _model(depth)._backbone.split
    _check(depth, V, B, hw)


# ---------------------------------------------------------------- 3. the head path at its threshold
def test_head_threshold_both_sides():
    split_launches = _check(18, 4, 86, 64)          # 1032 rows: the split Linears of _forward_split
    mfma_launches = _check(18, 4, 85, 64)           # 1020 rows: the generated-input fp32-MFMA Linears
    assert split_launches != mfma_launches


# ---------------------------------------------------------------- 4. MVG_SPLIT=0
@pytest.mark.parametrize("depth,V,B,hw", [(18, 2, 2, 64), (50, 2, 1, 64)])
def test_fp32_mfma_kernels_everywhere(depth, V, B, hw):
    m = _model(depth)
    imgs, rot = _inputs(B, V, hw)
    split_ref = _python(m, imgs, rot)
    m._backbone.split = False
    try:
        want = _python(m, imgs, rot)
        with _session(m, V, B, hw) as s:
            _same(s.run(imgs, rot), want)
    finally:
        m._backbone.split = True
    assert not torch.equal(want[0], split_ref[0])     # the two kernel families round differently: the switch reached the session


# ---------------------------------------------------------------- 5. the 2 GiB guard
def test_guard_is_evaluated_from_the_real_sizes(monkeypatch):
    from rot_mvgaze_amd import backbone as BB
    from rot_mvgaze_amd._lib import SessionCfg, lib
    m = _model(18)
    V, B, hw = 2, 2, 64
    imgs, rot = _inputs(B, V, hw)
    want = _python(m, imgs, rot)
    assert m._backbone._split_now
    monkeypatch.setattr(BB.Backbone, "_guard_scale", 10 ** 6)
    tripped = _python(m, imgs, rot)                   # the Python hook pushes this small shape off the split kernels ...
    assert not m._backbone._split_now
    with _session(m, V, B, hw) as s:                  # ... the session decides from the real sizes: still the split kernels
        got = s.run(imgs, rot)
    _same(got, want)
    assert not torch.equal(tripped[0], want[0])
    # a shape whose layer1 output does reach 2 GiB per view (R50, 224 px, B >= 668) leaves the split kernels: the plan loses
    # exactly the split of the pooled map (host only, nothing is allocated)
    n = {}
    for batch in (660, 700):
        h = C.c_void_p()
        cfg = SessionCfg(depth=50, num_iter=3, views=2, batch=batch, height=224, width=224, split=1)
        assert lib().mvg_session_create(C.byref(cfg), C.byref(h)) == 0
        n[batch] = lib().mvg_session_launches(h)
        lib().mvg_session_destroy(h)
    assert n[700] == n[660] - 1


# ---------------------------------------------------------------- 6. raw uint8 patches
def test_raw_u8_patches():
    m = _model(18)
    V, B, hw = 2, 2, 64
    rng = np.random.default_rng(3)
    u8 = [torch.from_numpy(rng.integers(0, 256, size=(B, 80, 72, 3), dtype=np.uint8)).to(dev()) for _ in range(V)]
    _, rot = _inputs(B, V, hw)
    old = (m.input_size, m.input_bgr)
    m.input_size, m.input_bgr = hw, True
    try:
        want = _python(m, u8, rot)
    finally:
        m.input_size, m.input_bgr = old
    with _session(m, V, B, hw, raw_hw=(80, 72), input_bgr=True) as s:
        _same(s.run(u8, rot), want)


# ---------------------------------------------------------------- 7. the variants that only change pointers / drop the rotation
@pytest.mark.parametrize("variant", [dict(share_weights=True), dict(ignore_rotmat=True)])
def test_variants(variant):
    _check(18, 2, 3, 64, **variant)


def test_unserved_models_raise():
    from rot_mvgaze_amd.model import FeatRotationSymm
    from rot_mvgaze_amd.session import InferenceSession
    for kw in (dict(encode_rotmat=True), dict(share_feature=True)):
        with pytest.raises(ValueError):
            InferenceSession(FeatRotationSymm(18, 3, **kw), 2, 2, 64, 64)
    m = _model(18)
    m.compute_dtype = torch.bfloat16
    try:
        with pytest.raises(ValueError):
            InferenceSession(m, 2, 2, 64, 64)
    finally:
        m.compute_dtype = torch.float32


# ---------------------------------------------------------------- 8. refresh after the weights changed
def test_refresh_follows_the_weights():
    m = _model(18, fresh=True)
    V, B, hw = 2, 3, 64
    imgs, rot = _inputs(B, V, hw)
    with _session(m, V, B, hw) as s:
        first = [o.clone() for o in s.run(imgs, rot)]
        _same(first, _python(m, imgs, rot))
        with torch.no_grad():
            m.param_arena().mul_(1.03125)             # every parameter, in place
        m.invalidate_weight_cache()                   # (the Python path's cached sp copies: the write bypassed the version counters)
        want = _python(m, imgs, rot)
        s.refresh()
        second = s.run(imgs, rot)
        _same(second, want)
        assert not torch.equal(second[3], first[3]) and not torch.equal(second[0], first[0])


# ---------------------------------------------------------------- 9. sessions share a model; a session repeats itself
def test_two_sessions_on_one_model():
    m = _model(18)
    ia, ra = _inputs(3, 2, 64)
    ib, rb = _inputs(2, 3, 96, seed=77)
    wa, wb = _python(m, ia, ra), _python(m, ib, rb)
    with _session(m, 2, 3, 64) as a, _session(m, 3, 2, 96) as b:
        ga = [o.clone() for o in a.run(ia, ra)]
        gb = [o.clone() for o in b.run(ib, rb)]
        ga2 = a.run(ia, ra)
        _same(ga, wa)
        _same(gb, wb)
        _same(ga2, ga)
        _same(_python(m, ia, ra), wa)                 # and the module is undisturbed (its scratch registration, its caches)


# ---------------------------------------------------------------- 10. nothing but launches
def test_run_does_not_synchronise_or_allocate():
    m = _model(18)
    V, B, hw = 2, 3, 64
    imgs, rot = _inputs(B, V, hw)
    want = _python(m, imgs, rot)
    with _session(m, V, B, hw) as s:
        out = s.empty_outputs()
        s.run(imgs, rot, out=out)                     # warm-up
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for _ in range(10):
                s.run(imgs, rot, out=out)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.cuda.memory_allocated() == before
        torch.cuda.synchronize()
        _same(out, want)
