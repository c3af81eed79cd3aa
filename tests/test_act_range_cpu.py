"""CPU-side checks of the backbone activations' per-tensor scales (training steps on the split kernels): the new entry
points are declared in include/rotmvgaze.h beside the unchanged ones they extend (exported and bound: tests/test_cabi_cpu.py,
for every function) and wrapped in ops; and the bound chain itself - evaluated on the host by tests/act_range_ref.py - leaves every tensor of the networks
the tests and the benchmark build UNSCALED (the dead band 1 <= bound < 2^15: those networks keep their bits) and gives
the modified networks of tests/test_act_range_gpu.py the power of two the formula says."""
import math

import numpy as np
import pytest

import cabi_header as hdr
import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd.arch import backbone_spec
from act_range_ref import P, RANGE_CASES, RANGE_IDS, expected_bounds, expected_sinv, modified_state_dict, sinv_for

NAMES = ("mvg_act_scales", "mvg_bn_apply_split_scaled", "mvg_bn_relu_maxpool_fwd_split_scaled", "mvg_avgpool_fwd_split_scaled",
         "mvg_conv_wgrad_split_xs", "mvg_conv_wgrad_split_slabs_xs")
# the entry points these extend keep their signatures (the ABI version does not move)
UNCHANGED = {"mvg_bn_apply_split": 14, "mvg_bn_relu_maxpool_fwd_split": 13, "mvg_avgpool_fwd_split": 6, "mvg_conv_wgrad_split": 9,
             "mvg_conv_wgrad_split_slabs": 7, "mvg_conv_fprop_split": 8}


def test_act_scale_entry_points_declared_exported_and_bound():
    for name in NAMES + tuple(UNCHANGED):
        assert name in hdr.functions, f"{name} is not declared in include/rotmvgaze.h"
    for name, nargs in UNCHANGED.items():
        assert hdr.arity(name) == nargs, f"{name} changed its signature"


def test_act_scale_ops_wrappers_exist():
    from rot_mvgaze_amd import ops
    for fn in ("act_scales", "bn_apply_split", "bn_relu_maxpool_fwd_split", "avgpool_fwd_split", "conv_wgrad_split"):
        assert callable(getattr(ops, fn))
    from rot_mvgaze_amd.backbone import Backbone
    assert callable(Backbone._prepare_act_scales)


def test_banded_scale_rule():
    assert sinv_for(1.0) == 1.0 and sinv_for(32767.9) == 1.0 and sinv_for(1901.0) == 1.0          # the dead band
    assert sinv_for(32768.0) == 2.0 and sinv_for(0.99) == 2.0 ** -15 and sinv_for(0.5) == 2.0 ** -15 and sinv_for(0.49) == 2.0 ** -16
    assert sinv_for(2.0 ** 16 * 100.0) == 2.0 ** 8                  # 100 * 2^16 = 0.78 * 2^23 -> k = -8
    for bad in (0.0, float("inf"), float("nan"), -1.0):
        assert sinv_for(bad) == 1.0
    for b in (3e-9, 0.7, 40000.0, 1e9, 3e30):                       # outside the band the bound lands in [2^14, 2^15)
        assert 2.0 ** 14 <= b / sinv_for(b) < 2.0 ** 15


@pytest.mark.parametrize("conditioned", [False, True])
@pytest.mark.parametrize("perturb_bn", [True, False])
@pytest.mark.parametrize("depth", [18, 50])
def test_unmodified_networks_stay_unscaled(depth, perturb_bn, conditioned):
    """Every sp activation of the seeded networks (the tests' perturbed recipe and the benchmark's plain one) has its bound
    inside [1, 2^15) at the tests' small sizes and at the benchmark's: every scale is exactly 1, so this feature does not
    change what those networks compute."""
    sd = modified_state_dict(depth, conditioned=conditioned, perturb_bn=perturb_bn)
    for B, px in ((2, 64), (8, 64), (64, 224), (128, 224)):
        bounds = expected_bounds(sd, depth, B, px, px)
        assert len(bounds) == {18: 17, 50: 49}[depth]              # one sp tensor per unit that is not a downsample branch
        lo, hi = min(bounds.values()), max(bounds.values())
        assert 1.0 <= lo and hi < 32768.0, (B, px, float(lo), float(hi))
        assert set(expected_sinv(sd, depth, B, px, px).values()) == {1.0}


@pytest.mark.parametrize("depth,batch,hw,conditioned,bn,factor", RANGE_CASES, ids=RANGE_IDS)
def test_modified_networks_get_the_scale_the_formula_gives(depth, batch, hw, conditioned, bn, factor):
    base = modified_state_dict(depth, conditioned=conditioned)
    sd = modified_state_dict(depth, bn, factor, conditioned=conditioned)
    b0, b1 = expected_bounds(base, depth, batch, hw, hw), expected_bounds(sd, depth, batch, hw, hw)
    s1 = expected_sinv(sd, depth, batch, hw, hw)
    # the tensor the modified BatchNorm bounds: its unit's output - for a downsample BatchNorm the output of its block
    spec = backbone_spec(depth)
    plain = {c.bn: c.name for blk in spec.blocks for c in blk.convs[:-1]}
    plain[spec.stem.bn] = spec.stem.name
    chained = {c.bn: blk.convs[-1].name for blk in spec.blocks for c in (blk.convs[-1], blk.downsample) if c is not None}
    conv = plain.get(P + bn) or chained[P + bn]
    moved = [k for k in b1 if b1[k] != b0[k]]
    assert conv in moved
    if P + bn in plain:                                          # a power of two: a unit's bound scales exactly
        assert float(b1[conv]) == float(b0[conv]) * factor
    # the scale, from float64 arithmetic on the modified parameters: bound just below 2^15
    k = -math.log2(s1[conv])
    assert k == round(k) and k != 0
    assert 2.0 ** 14 <= float(b1[conv]) * 2.0 ** k < 2.0 ** 15
    for name in b1:                                              # everything the modification does not reach stays unscaled
        if name not in moved:
            assert s1[name] == 1.0
    if factor > 1:      # today's failure: the bound is honest - the tensor really exceeds fp16's range somewhere near it
        assert float(b1[conv]) > 65504.0


def test_non_finite_parameters_give_scale_one():
    for bad in (np.inf, np.nan):
        for name, ch in (("layer2.0.bn1.weight", 3), ("layer1.1.bn2.bias", 0)):      # a plain unit; a block output (chained on)
            sd = modified_state_dict(18)
            a = sd[P + name].copy()
            a[ch] = bad
            sd[P + name] = a
            assert set(expected_sinv(sd, 18, 8, 64, 64).values()) == {1.0}
