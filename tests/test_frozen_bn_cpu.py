"""Frozen-BatchNorm training steps, on the host alone: the C ABI of the two bf16 entry points (declared with the fp32 entry
points' signatures, uint16_t for every activation-typed pointer; exported and bound type for type: tests/test_cabi_cpu.py checks
that for every function), the ABI version, and backbone.plan_call's train_step keyword."""
import itertools

import pytest

import cabi_header as hdr
import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd import _lib
from rot_mvgaze_amd.arch import backbone_spec
from rot_mvgaze_amd.backbone import Call, Family, plan_call, unit_family

R18, R50 = backbone_spec(18), backbone_spec(50)
PAIRS = (("mvg_bn_eval_bwd", "mvg_bn_eval_bwd_bf16"), ("mvg_bn_relu_maxpool_eval_bwd", "mvg_bn_relu_maxpool_eval_bwd_bf16"))


def test_bf16_entry_points_have_the_fp32_signatures():
    for f32, b16 in PAIRS:
        assert b16 in hdr.functions, f"{b16} is not declared in include/rotmvgaze.h"
        (ret32, args32), (ret16, args16) = hdr.functions[f32], hdr.functions[b16]
        assert ret16 == ret32 == "int"
        assert [n for _, n in args16] == [n for _, n in args32]
        act = {"g", "act", "y", "dy", "dz_out", "g_pooled"}
        for (t32, n), (t16, _) in zip(args32, args16):
            assert t16 == ("uint16_t*" if n in act else t32), (b16, n, t16)
            assert n not in act or t32 == "float*"
    assert hdr.parameter_names("mvg_bn_eval_bwd_bf16")[:4] == ["g", "act", "relu_bits", "y"]
    assert hdr.parameter_names("mvg_bn_relu_maxpool_eval_bwd_bf16")[:3] == ["g_pooled", "argmax", "y"]


def test_symbols_are_exported_bound_and_wrapped():
    from rot_mvgaze_amd import ops
    L = _lib.lib()
    for f32, b16 in PAIRS:
        assert callable(getattr(L, b16))
        assert getattr(L, b16).argtypes == getattr(L, f32).argtypes
    assert callable(ops.bn_eval_bwd) and callable(ops.bn_relu_maxpool_eval_bwd)


def test_abi_version_is_13():
    assert hdr.constants["MVG_ABI_VERSION"] == 13 == _lib.ABI_VERSION == _lib.lib().mvg_abi_version()


def plan(spec=R50, B=2, hw=224, H=None, W=None, training=True, keep_tape=True, **kw):
    return plan_call(spec, V=2, B=B, H=hw if H is None else H, W=hw if W is None else W, training=training, keep_tape=keep_tape, **kw)


def test_train_step_is_the_last_field_and_defaults_to_training():
    assert Call._fields[-1] == "train_step" and "train_step" in Call._field_defaults
    for training, keep in itertools.product((True, False), (True, False)):
        assert plan(training=training, keep_tape=keep).train_step is training
        assert plan(training=training, keep_tape=keep, bf16=True, hw=64).train_step is training


# every argument set tests/test_backbone_call_cpu.py plans with
_PER_IMAGE = 4 * 56 * 56 * 256
_EDGE = (0x7FFFFFF0 - 1) // _PER_IMAGE
_WEDGE = (0x7FFFFFF0 - 1) // (32 * 224 * 112 * 4)
_INFER = dict(training=False, keep_tape=False)
ARGSETS = [
    dict(B=_EDGE), dict(B=_EDGE + 1), dict(B=_EDGE, **_INFER), dict(B=_EDGE + 1, **_INFER),
    dict(B=1, guard_scale=_EDGE), dict(B=1, guard_scale=_EDGE + 1), dict(B=2), dict(B=2, guard_scale=10 ** 6),
    dict(), dict(W=223), dict(need_dimg=True), dict(batch_weight_prep=False), dict(stem_rowwindow=False), dict(split=False),
    dict(training=False), dict(spec=R18, B=_WEDGE), dict(spec=R18, B=_WEDGE + 1),
    dict(bf16=True, hw=64), dict(bf16=True, H=64, W=66), dict(bf16=True, hw=72), dict(bf16=True, B=16, hw=72),
    dict(bf16=True, hw=64, training=False), dict(bf16=True, hw=64, batch_weight_prep=False), dict(bf16=True, hw=64, stem_rowwindow=False),
    dict(bf16=True, hw=64, need_dimg=True), dict(bf16=True),
    dict(training=True, split_eval_guard="fallback", capturing=True),
    dict(bf16=True, hw=64, raw=True, training=True, keep_tape=True, augment=True), dict(bf16=True, hw=64, raw=True, **_INFER),
    dict(**_INFER), dict(split_eval_guard="record", **_INFER), dict(split_eval_guard="record"),
    dict(split_eval_guard="record", split_eval=False, **_INFER), dict(split_eval_guard="fallback", tripped=True, **_INFER),
    dict(split_eval_guard="record", tripped=True, **_INFER),
    dict(spec=R18), dict(spec=R18, stem_rowwindow=False), dict(spec=R18, **_INFER), dict(spec=R18, split=False),
    dict(spec=R18, split_eval=False, **_INFER), dict(spec=R18, training=False, keep_tape=True),
    dict(spec=R18, bf16=True, hw=64), dict(spec=R18, bf16=True, **_INFER), dict(spec=R18, bf16=True, bf16_fold_eval=False, **_INFER),
    dict(bf16=True, **_INFER), dict(bf16=True, bf16_fold_eval=False, **_INFER),
]


@pytest.mark.parametrize("i", range(len(ARGSETS)))
def test_default_keyword_changes_nothing(i):
    """Leaving train_step out is passing the BatchNorm flag: the same record, and every field but the new one is what the
    decisions of the record's other fields say it was before the keyword existed (they never read it with the default)."""
    kw = dict(ARGSETS[i])
    training = kw.get("training", True)
    a, b = plan(**kw), plan(**kw, train_step=training)
    assert a == b and a.train_step is training
    # the keyword moves nothing but itself where no raw patches are involved
    if not kw.get("raw"):
        c = plan(**kw, train_step=not training)
        assert c._replace(train_step=training) == a


def test_refusals_with_the_default_keep_their_cases():
    for training, keep_tape, augment in ((True, True, False), (False, True, False), (False, True, True)):
        with pytest.raises(NotImplementedError, match="raw uint8 input with the bf16 path is served for inference only"):
            plan(bf16=True, hw=64, raw=True, training=training, keep_tape=keep_tape, augment=augment)


@pytest.mark.parametrize("spec", [R18, R50], ids=["r18", "r50"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_a_frozen_step_plans_a_taped_call_without_statistics(spec, bf16):
    """training False, train_step True: taped, no row-window stem, no sp storage - the taped eval forward's kernels (fp32-MFMA,
    or bf16) - for both dtypes, at sizes where the train-mode step has a row-window stem."""
    train = plan(spec, bf16=bf16, hw=64)
    assert train.stem_rw and train.train_step and train.training
    fr = plan(spec, bf16=bf16, hw=64, training=False, train_step=True)
    assert fr.taped and not fr.stem_rw and not fr.sp and fr.train_step is True and fr.training is False
    want = Family.BF16 if bf16 else Family.FP32
    assert {unit_family(fr, c) for c in spec.all_convs()} == {want}
    assert fr == plan(spec, bf16=bf16, hw=64, training=False)._replace(train_step=True)      # the eval tape's plan, but a step
    # without a tape (torch.no_grad() inside train()): the folded inference forward, as in eval mode
    nf = plan(spec, bf16=bf16, hw=64, training=False, keep_tape=False, train_step=True)
    assert not nf.taped and nf.sp == (not bf16)


def test_a_frozen_step_takes_raw_patches_with_an_augment_on_the_bf16_path():
    fr = plan(bf16=True, hw=64, raw=True, augment=True, training=False, train_step=True)
    assert fr.taped and not fr.stem_rw and fr.train_step
    plan(bf16=True, hw=64, raw=True, augment=True, training=False, keep_tape=False, train_step=True)
    with pytest.raises(NotImplementedError, match="raw uint8 input with the bf16 path is served for inference only"):
        plan(bf16=True, hw=64, raw=True, augment=False, training=False, train_step=True)
    # the eval-mode tape with an augment set is no training step: refused as before
    with pytest.raises(NotImplementedError, match="inference only"):
        plan(bf16=True, hw=64, raw=True, augment=True, training=False, train_step=False)
    # the fp32 model takes raw patches in every mode
    assert not plan(hw=64, raw=True, augment=True, training=False, train_step=True).sp
