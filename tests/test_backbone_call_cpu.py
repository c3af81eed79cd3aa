"""backbone.plan_call and backbone.unit_family: the size and mode decisions of one Backbone.forward call and the kernel family
of every conv, on the host alone (no device, no tensor)."""
import dataclasses

import pytest

from rot_mvgaze_amd.arch import backbone_spec
from rot_mvgaze_amd.backbone import Family, plan_call, unit_family

R18, R50 = backbone_spec(18), backbone_spec(50)
LIMIT = 0x7FFFFFF0                      # the 32-bit offset bound of the split kernels, in bytes


def plan(spec=R50, B=2, hw=224, H=None, W=None, training=True, keep_tape=True, **kw):
    return plan_call(spec, V=2, B=B, H=hw if H is None else H, W=hw if W is None else W, training=training, keep_tape=keep_tape, **kw)


def test_two_gib_guard_at_its_real_edge():
    # ResNet-50 at 224 x 224: layer1's output is 56 x 56 x 256 per image, 4 bytes per sp element
    per_image = 4 * 56 * 56 * R50.blocks[0].convs[-1].cout
    edge = (LIMIT - 1) // per_image                 # the largest batch whose view stays below the bound
    assert edge == 668 and per_image * edge < LIMIT <= per_image * (edge + 1)
    on, off = plan(B=edge), plan(B=edge + 1)
    assert on.split and on.sp and not off.split and not off.sp
    assert unit_family(on, R50.blocks[0].convs[0]) is Family.SPLIT
    assert {unit_family(off, c) for c in R50.all_convs()} == {Family.FP32}
    assert not off.stem_rw
    # inference is held to the same bound
    assert plan(B=edge, training=False, keep_tape=False).sp and not plan(B=edge + 1, training=False, keep_tape=False).sp


def test_guard_scale_moves_the_edge():
    per_image = 4 * 56 * 56 * 256
    edge = (LIMIT - 1) // per_image
    assert plan(B=1, guard_scale=edge).split and not plan(B=1, guard_scale=edge + 1).split
    assert plan(B=2).split and not plan(B=2, guard_scale=10 ** 6).split


def test_split_stem_form():
    assert plan().stem_rw and unit_family(plan(), R50.stem) is Family.SPLIT
    for off in (plan(W=223), plan(need_dimg=True), plan(batch_weight_prep=False), plan(stem_rowwindow=False), plan(split=False),
                plan(training=False)):
        assert not off.stem_rw
    assert unit_family(plan(need_dimg=True), R50.stem) is Family.FP32 and plan(need_dimg=True).sp
    # the window tensor's own 32-bit bound: 32 channels x B x H x W/2 sp elements.  ResNet-18's layer1 is 64 wide, so the
    # 2 GiB guard of the call still holds where the windows no longer fit
    window_bytes = 32 * 224 * 112 * 4
    edge = (LIMIT - 1) // window_bytes
    on, off = plan(R18, B=edge), plan(R18, B=edge + 1)
    assert on.split and on.stem_rw and off.split and not off.stem_rw


def test_bf16_stem_form():
    assert plan(bf16=True, hw=64).stem_rw
    assert not plan(bf16=True, H=64, W=66).stem_rw                       # W % 4
    assert 2 * 36 * 18 % 64 != 0 and not plan(bf16=True, hw=72).stem_rw  # B ho (wo / 2) partial rows: no multiple of 64
    assert plan(bf16=True, B=16, hw=72).stem_rw                          # (16 * 36 * 18 is one)
    k5 = dataclasses.replace(R50, stem=dataclasses.replace(R50.stem, k=5, pad=2))
    assert not plan(k5, bf16=True, hw=64).stem_rw
    for off in (plan(bf16=True, hw=64, training=False), plan(bf16=True, hw=64, batch_weight_prep=False),
                plan(bf16=True, hw=64, stem_rowwindow=False)):
        assert not off.stem_rw
    assert plan(bf16=True, hw=64, need_dimg=True).stem_rw                # (the backward refuses d(img) on this path)
    assert not plan(bf16=True).sp


def test_errors_keep_their_messages():
    with pytest.raises(ValueError, match=r"split_eval_guard must be None, 'record' or 'fallback' \(got 'always'\)"):
        plan(split_eval_guard="always")
    with pytest.raises(RuntimeError, match="split_eval_guard = 'fallback' reads the range record on the host and cannot run while "
                                           "the stream is capturing"):
        plan(training=False, keep_tape=False, split_eval_guard="fallback", capturing=True)
    plan(training=True, split_eval_guard="fallback", capturing=True)     # (the guard covers folded fp32 inference only)
    for training, keep_tape, augment in ((True, True, False), (False, True, False), (False, True, True)):
        with pytest.raises(NotImplementedError, match="raw uint8 input with the bf16 path is served for inference only"):
            plan(bf16=True, hw=64, raw=True, training=training, keep_tape=keep_tape, augment=augment)
    plan(bf16=True, hw=64, raw=True, training=True, keep_tape=True, augment=True)
    plan(bf16=True, hw=64, raw=True, training=False, keep_tape=False)


def test_range_guard_of_the_call():
    infer = dict(training=False, keep_tape=False)
    assert plan(**infer).guard is None and not plan(**infer).range_live
    assert plan(split_eval_guard="record", **infer).range_live
    assert plan(split_eval_guard="record").guard is None                 # a taped call ignores it
    assert not plan(split_eval_guard="record", split_eval=False, **infer).range_live
    tripped = plan(split_eval_guard="fallback", tripped=True, **infer)
    assert not tripped.split and not tripped.sp and not tripped.range_live
    assert plan(split_eval_guard="record", tripped=True, **infer).split  # only "fallback" stays on the fp32-MFMA kernels


@pytest.mark.parametrize("spec", [R18, R50], ids=["r18", "r50"])
def test_unit_family_over_every_conv(spec):
    convs = spec.all_convs()
    assert convs[0] is spec.stem and len(convs) == (20 if spec.depth == 18 else 53)
    rest = convs[1:]
    # an fp32 training call on the split kernels: every conv but the 3-channel stem, and the stem in row-window form
    call = plan(spec)
    assert unit_family(call, spec.stem) is Family.SPLIT and all(unit_family(call, c) is Family.SPLIT for c in rest)
    call = plan(spec, stem_rowwindow=False)
    assert unit_family(call, spec.stem) is Family.FP32 and call.sp and all(unit_family(call, c) is Family.SPLIT for c in rest)
    # folded inference on the split kernels: the stem on the fp32-MFMA kernel, its pooled map stored in sp
    call = plan(spec, training=False, keep_tape=False)
    assert unit_family(call, spec.stem) is Family.FP32 and call.sp and all(unit_family(call, c) is Family.SPLIT for c in rest)
    # fp32-MFMA calls: MVG_SPLIT=0, split_eval off, eval mode with a tape
    for call in (plan(spec, split=False), plan(spec, training=False, keep_tape=False, split_eval=False),
                 plan(spec, training=False, keep_tape=True)):
        assert not call.sp and all(unit_family(call, c) is Family.FP32 for c in convs)
    # bf16 calls: training, folded and unfolded inference
    for call in (plan(spec, bf16=True, hw=64), plan(spec, bf16=True, training=False, keep_tape=False),
                 plan(spec, bf16=True, training=False, keep_tape=False, bf16_fold_eval=False)):
        assert not call.sp and all(unit_family(call, c) is Family.BF16 for c in convs)


def test_the_call_record_is_frozen_and_names_its_path():
    call = plan()
    with pytest.raises(AttributeError):
        call.split = False
    assert call.taped and plan(training=False, keep_tape=True).taped and not plan(training=False, keep_tape=False).taped
    assert not plan(bf16=True, training=False, keep_tape=False).taped
    assert plan(bf16=True, training=False, keep_tape=False, bf16_fold_eval=False).taped
    assert (call.V, call.B, call.H, call.W, call.boundary, call.wprep, call.act_sinv) == (2, 2, 224, 224, -1, None, None)
