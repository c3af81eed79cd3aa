"""Which block outputs are formed inside the next block's conv1 forward launch (backbone.bn_apply_fprop_eligible /
bn_apply_fprop_pairs): decided from the architecture plan and the mode alone, no GPU.  And the new C entries' declarations."""
import cabi_header as hdr
import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd.arch import ConvSpec, backbone_spec
from rot_mvgaze_amd.backbone import Backbone, bn_apply_fprop_eligible, bn_apply_fprop_pairs

P = "_feat_extractor.0."
R50_PAIRS = [(P + "layer1.0.conv3", P + "layer1.1.conv1"), (P + "layer1.1.conv3", P + "layer1.2.conv1"),
             (P + "layer1.2.conv3", P + "layer2.0.conv1"), (P + "layer2.0.conv3", P + "layer2.1.conv1"),
             (P + "layer2.1.conv3", P + "layer2.2.conv1"), (P + "layer2.2.conv3", P + "layer2.3.conv1")]


def test_resnet50_takes_exactly_the_six_pairs_of_layer1_and_layer2():
    spec = backbone_spec(50)
    got = bn_apply_fprop_pairs(spec)
    assert got == R50_PAIRS                      # forward order
    by_name = {c.name: c for b in spec.blocks for c in b.convs}
    assert [(by_name[b].cin, by_name[b].cout) for _, b in got] == [(256, 64)] * 2 + [(256, 128)] + [(512, 128)] * 3
    # the two whose residual is the raw downsample output (the affine form) are among them
    ds = {b.convs[-1].name for b in spec.blocks if b.downsample is not None}
    assert [a for a, _ in got if a in ds] == [P + "layer1.0.conv3", P + "layer2.0.conv3"]


def test_resnet18_takes_none():
    assert bn_apply_fprop_pairs(backbone_spec(18)) == []


def test_other_paths_take_none():
    spec = backbone_spec(50)
    assert bn_apply_fprop_pairs(spec, bf16=True) == []
    assert bn_apply_fprop_pairs(spec, training=False) == []          # eval-mode BatchNorm: no batch statistics
    assert bn_apply_fprop_pairs(spec, split=False) == []             # MVG_SPLIT=0: the fp32-MFMA kernels
    assert bn_apply_fprop_pairs(spec, enabled=False) == []           # the switch off
    assert bn_apply_fprop_pairs(spec, single_stage=lambda c: False) == []
    # a small batch: the launch plan pipelines the 128-column consumers, the 64-column ones stay single-stage
    assert bn_apply_fprop_pairs(spec, single_stage=lambda c: c.cout == 64) == R50_PAIRS[:2]


def test_pair_predicate_conditions():
    ok = dict(split=True, trained=True, residual=True, relu=True, single_stage=True)
    prod, cons = ConvSpec("a.conv3", "a.bn3", 64, 256, 1, 1, 0), ConvSpec("b.conv1", "b.bn1", 256, 64, 1, 1, 0)
    assert bn_apply_fprop_eligible(prod, cons, **ok)
    for k in ok:
        assert not bn_apply_fprop_eligible(prod, cons, **{**ok, k: False}), k
    assert bn_apply_fprop_eligible(ConvSpec("a", "b", 128, 512, 1, 1, 0), ConvSpec("c", "d", 512, 128, 1, 1, 0), **ok)
    for p2, c2 in ((prod, ConvSpec("c", "d", 256, 256, 1, 1, 0)),                                       # two column tiles
                   (prod, ConvSpec("c", "d", 256, 64, 3, 1, 1)),
                   (prod, ConvSpec("c", "d", 256, 64, 1, 2, 0)),
                   (prod, ConvSpec("c", "d", 256, 96, 1, 1, 0)),
                   (prod, ConvSpec("c", "d", 128, 64, 1, 1, 0)),                                        # not this producer's output
                   (ConvSpec("a", "b", 256, 1024, 1, 1, 0), ConvSpec("c", "d", 1024, 128, 1, 1, 0)),    # beyond the constants' table
                   (ConvSpec("a", "b", 16, 48, 1, 1, 0), ConvSpec("c", "d", 48, 64, 1, 1, 0))):         # cin % 32
        assert not bn_apply_fprop_eligible(p2, c2, **ok), (p2, c2)


def test_switch_defaults_on():
    assert Backbone(50, {}).fuse_bn_apply_fprop is True


def test_new_entries_are_declared_and_have_signatures():
    for name, nargs in (("mvg_conv_fprop_split_bnapply", 17), ("mvg_conv_fprop_split_stages", 1)):
        assert name in hdr.functions, name + " is not declared in include/rotmvgaze.h"
        assert hdr.functions[name][0] == "int" and hdr.arity(name) == nargs
