"""Frozen-BatchNorm training steps on the split kernels (Backbone.split_frozen), on the host alone: what plan_call decides with
the flag, and the activation bound the scales of such a step come from (tests/frozen_split_ref.py) against float64 truth.

The bound's bars are not tolerances: a bound holds (>= the largest |value|, in float64) or it does not."""
import itertools

import numpy as np
import pytest

import frozen_split_ref as ref
import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd.arch import backbone_spec
from rot_mvgaze_amd.backbone import Call, Family, frozen_split, plan_call, unit_family

R18, R50 = backbone_spec(18), backbone_spec(50)
EPS = 1e-5
FROZEN = dict(training=False, keep_tape=True, train_step=True)


def plan(spec=R50, B=2, hw=224, H=None, W=None, training=True, keep_tape=True, **kw):
    return plan_call(spec, V=2, B=B, H=hw if H is None else H, W=hw if W is None else W, training=training, keep_tape=keep_tape, **kw)


# ---------------------------------------------------------------- plan_call
@pytest.mark.parametrize("spec", [R18, R50], ids=["r18", "r50"])
def test_a_flagged_frozen_step_runs_every_conv_on_the_split_kernels(spec):
    call = plan(spec, split_frozen=True, **FROZEN)
    assert call.sp and call.stem_rw and call.split and call.taped and frozen_split(call)
    assert call.training is False and call.train_step is True and call.guard is None and not call.range_live
    assert all(unit_family(call, c) is Family.SPLIT for c in spec.all_convs())
    # the stem's form follows the conditions of a train-mode step: an odd width, no batched weight prep -> fp32-MFMA taps, sp kept
    for kw in (dict(W=223), dict(batch_weight_prep=False), dict(stem_rowwindow=False)):
        c2, tr = plan(spec, split_frozen=True, **FROZEN, **kw), plan(spec, **kw)
        assert c2.sp and c2.stem_rw is False and tr.stem_rw is False
        assert unit_family(c2, spec.stem) is Family.FP32
        assert all(unit_family(c2, c) is Family.SPLIT for c in spec.all_convs() if c.cin != 3)
    # and equals the train-mode plan in everything but the two mode fields
    tr = plan(spec)
    assert call._replace(training=True) == tr._replace(train_step=True)


EXCLUDED = {
    "eval-mode tape": dict(training=False, keep_tape=True),
    "eval-mode tape, train_step False": dict(training=False, keep_tape=True, train_step=False),
    "need_dimg": dict(need_dimg=True, **FROZEN),
    "bf16": dict(bf16=True, hw=64, **FROZEN),
    "MVG_SPLIT=0": dict(split=False, **FROZEN),
    "2 GiB guard": dict(guard_scale=10 ** 6, **FROZEN),
    "no tape": dict(training=False, keep_tape=False, train_step=True),
    "folded inference": dict(training=False, keep_tape=False),
    "train mode": dict(training=True, keep_tape=True),
    "train mode, no tape": dict(training=True, keep_tape=False),
}


@pytest.mark.parametrize("name", sorted(EXCLUDED))
def test_the_flag_is_inert_everywhere_else(name):
    kw = EXCLUDED[name]
    on, off = plan(split_frozen=True, **kw), plan(**kw)
    assert on == off, name
    assert not frozen_split(on)
    if name not in ("folded inference", "no tape", "train mode", "train mode, no tape"):      # (those store in sp for reasons of their own)
        assert not on.sp and not on.stem_rw or on.bf16


def test_with_the_flag_off_a_frozen_step_plans_what_it_did():
    """Field for field: the record of a frozen step as the parent planned it (tests/test_frozen_bn_cpu.py and
    tests/test_frozen_bn_gpu.py hold the same facts), with the keyword absent and with its default."""
    for spec, B, hw in itertools.product((R18, R50), (2, 32), (64, 224)):
        a, b = plan(spec, B=B, hw=hw, **FROZEN), plan(spec, B=B, hw=hw, split_frozen=False, **FROZEN)
        want = Call(V=2, B=B, H=hw, W=hw, training=False, keep_tape=True, bf16=False, split=True, sp=False, stem_rw=False, taped=True,
                    guard=None, range_live=False, need_dimg=False, boundary=-1, wprep=None, act_sinv=None, train_step=True)
        assert a == b == want
        assert all(unit_family(a, c) is Family.FP32 for c in spec.all_convs())
    assert Call._fields[-1] == "train_step"


# ---------------------------------------------------------------- the bound
def _unit(rng, G, rows, c, shift=3.0, shrink=0.05):
    """Random conv outputs with per-channel offsets and spreads, gamma / beta of both signs, and running statistics that do NOT
    describe them: the running mean shifted by `shift` spreads, the running variance shrunken to `shrink` of the batch's."""
    spread = np.exp(rng.standard_normal(c))
    y = (rng.standard_normal((G, rows, c)) * spread + rng.standard_normal(c) * 2).astype(np.float32)
    gamma = (rng.standard_normal(c) * 1.5).astype(np.float32)
    beta = rng.standard_normal(c).astype(np.float32)
    rm = (y.mean((0, 1)) + shift * spread * rng.choice([-1.0, 1.0], c)).astype(np.float32)
    rv = (y.var((0, 1)) * shrink).astype(np.float32)
    return y, gamma, beta, rm, rv


@pytest.mark.parametrize("G,rows,c", [(1, 2, 8), (2, 98, 32), (3, 1000, 64), (2, 7, 16)])
def test_the_bound_holds_in_float64(G, rows, c):
    rng = np.random.default_rng(100 * rows + c)
    y, gamma, beta, rm, rv = _unit(rng, G, rows, c)
    out = ref.normalised(y, gamma, beta, rm, rv, EPS)
    per = ref.unit_bound_per_channel(y, gamma, beta, rm, rv, EPS)
    true = np.abs(out).max(1)
    print(f"FROZEN-SPLIT bound g{G}_r{rows}_c{c}: tightest channel true / bound = {float((true / per).max()):.4f}")
    assert (per >= true).all()
    assert ref.unit_bound(y, gamma, beta, rm, rv, EPS) >= np.abs(out).max()
    # an outlier is where the inequality is tight: one row far away, every other one equal
    y2 = np.zeros((1, rows, c), np.float32)
    y2[0, 0] = 1000.0
    out2 = ref.normalised(y2, gamma, beta, np.zeros(c, np.float32), rv, EPS)
    b2 = ref.unit_bound_per_channel(y2, gamma, beta, np.zeros(c, np.float32), rv, EPS)
    assert (b2 * (1 + 1e-12) >= np.abs(out2).max(1)).all()
    assert (b2 <= np.abs(out2).max(1) * 1.0001 + 2 * np.abs(beta.astype(np.float64))).all()     # and no looser than that there


def test_the_chained_bound_holds_for_a_block_output():
    """A residual block: identity = relu(unit A) (a bound of its own), output = relu(unit B + identity); then a second block
    whose identity is the first one's output, and one with a downsample unit (no ReLU) as its identity."""
    rng = np.random.default_rng(7)
    G, rows, c = 2, 98, 32
    ua, ub, uc, ud = (_unit(rng, G, rows, c) for _ in range(4))
    relu = lambda t: np.maximum(t, 0.0)
    a = relu(ref.normalised(*ua, EPS))
    ba = ref.unit_bound(*ua, EPS)
    assert ba >= a.max()
    out1 = relu(ref.normalised(*ub, EPS) + a)
    b1 = ref.unit_bound(*ub, EPS) + ba
    assert b1 >= np.abs(out1).max()
    out2 = relu(ref.normalised(*uc, EPS) + out1)
    b2 = ref.unit_bound(*uc, EPS) + b1
    assert b2 >= np.abs(out2).max()
    ds = ref.normalised(*ud, EPS)                      # the downsample branch: both signs survive
    out3 = relu(ref.normalised(*uc, EPS) + ds)
    assert ref.unit_bound(*uc, EPS) + ref.unit_bound(*ud, EPS) >= np.abs(out3).max()


def test_the_scale_follows_the_2_to_the_15_rule():
    for b in (1.0, 1.5, 100.0, 32767.9, float(np.nextafter(np.float32(32768.0), np.float32(0)))):
        assert ref.scale_for(b) == 1.0
    for b in (32768.0, 65520.0, 1e6, 3.1e9, 0.99, 0.5, 1e-3, 2.0 ** -60, 1e30):
        s = ref.scale_for(b)
        assert s != 1.0 and np.log2(s) == int(np.log2(s))
        assert 2.0 ** 14 <= b * s < 2.0 ** 15, (b, s)
    for b in (0.0, -1.0, float("inf"), float("nan"), 3.1e38):
        assert ref.scale_for(b) == 1.0
    assert ref.sinv_for(65536.0) == 4.0 and ref.sinv_for(0.25) == 2.0 ** -16
    # a tensor scaled by the rule stays a factor of two below fp16's overflow point, margin included
    for b in (32768.0, 1e6, 7.3e12):
        assert b * ref.MARGIN * ref.scale_for(b * ref.MARGIN) < 65520.0 / 2 * 1.0001


def test_partials_restate_the_statistics():
    """The record the kernel reads, merged in float64 (Chan), gives the tensor's own mean and biased variance."""
    rng = np.random.default_rng(3)
    y = _unit(rng, 2, 98, 32)[0]
    st = ref.partials(y, 40).astype(np.float64)            # 40 + 40 + 18 rows
    assert st.shape == (2, 3, 2, 32)
    cnt = np.array([40, 40, 18], np.float64)[None, :, None]
    mean = st[:, :, 0].sum(1) / 98
    m2 = st[:, :, 1].sum(1) + (cnt * (st[:, :, 0] / cnt - mean[:, None]) ** 2).sum(1)
    np.testing.assert_allclose(mean, y.astype(np.float64).mean(1), rtol=0, atol=1e-5)
    np.testing.assert_allclose(m2 / 98, y.astype(np.float64).var(1), rtol=1e-5)
