"""Which units form their BatchNorm-backward dy inside their own backward-data launch (backbone.bn_apply_dgrad_eligible /
bn_apply_dgrad_units): decided from the architecture plan and the mode alone, no GPU."""
import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd.arch import ConvSpec, backbone_spec
from rot_mvgaze_amd.backbone import Backbone, bn_apply_dgrad_eligible, bn_apply_dgrad_units

P = "_feat_extractor.0."
R50_UNITS = [P + "layer2.%d.conv3" % i for i in (3, 2, 1, 0)] + [P + "layer1.%d.conv3" % i for i in (2, 1, 0)]


def test_resnet50_takes_exactly_the_seven_expand_units_of_layer1_and_layer2():
    spec = backbone_spec(50)
    got = bn_apply_dgrad_units(spec)
    assert got == R50_UNITS                      # backward order
    by_name = {c.name: c for b in spec.blocks for c in b.convs}
    assert sorted((by_name[n].cin, by_name[n].cout) for n in got) == [(64, 256)] * 3 + [(128, 512)] * 4


def test_resnet18_takes_none():
    assert bn_apply_dgrad_units(backbone_spec(18)) == []


def test_other_paths_take_none():
    spec = backbone_spec(50)
    assert bn_apply_dgrad_units(spec, bf16=True) == []
    assert bn_apply_dgrad_units(spec, split=False) == []             # MVG_SPLIT=0: the fp32-MFMA kernels
    assert bn_apply_dgrad_units(spec, training=False) == []          # eval-mode tape: frozen statistics
    assert bn_apply_dgrad_units(spec, need_dimg=True) == []
    assert bn_apply_dgrad_units(spec, fuse_bn_split=False) == []     # no fused reduce: no sums arrive with the gradient
    assert bn_apply_dgrad_units(spec, enabled=False) == []


def test_unit_predicate_conditions():
    ok = dict(split=True, trained=True, fused_in=True, carries_reduce=True)
    c = ConvSpec("x.conv3", "x.bn3", 64, 256, 1, 1, 0)
    assert bn_apply_dgrad_eligible(c, **ok)
    for k in ok:
        assert not bn_apply_dgrad_eligible(c, **{**ok, k: False}), k
    assert not bn_apply_dgrad_eligible(c, need_dimg=True, **ok)
    assert bn_apply_dgrad_eligible(ConvSpec("x", "y", 128, 512, 1, 1, 0), **ok)
    assert bn_apply_dgrad_eligible(ConvSpec("x", "y", 128, 160, 1, 1, 0), **ok)
    for bad in (ConvSpec("x", "y", 256, 1024, 1, 1, 0),      # layer3 conv3: two column tiles
                ConvSpec("x", "y", 512, 2048, 1, 1, 0),
                ConvSpec("x", "y", 32, 256, 1, 1, 0),
                ConvSpec("x", "y", 64, 64, 3, 1, 1),
                ConvSpec("x", "y", 128, 512, 1, 2, 0),
                ConvSpec("x", "y", 64, 48, 1, 1, 0),
                ConvSpec("x", "y", 128, 1024, 1, 1, 0)):     # constants beyond the kernel's table
        assert not bn_apply_dgrad_eligible(bad, **ok), bad


def test_switch_defaults_on():
    assert Backbone(50, {}).fuse_bn_apply_dgrad is True
