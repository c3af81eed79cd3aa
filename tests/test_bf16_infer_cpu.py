"""CPU-side checks of the bf16 inference path's boundary: the header declares the new entry points with the
argument lists of their fp32 twins (how every function is exported and bound: tests/test_cabi_cpu.py), and the backbone
exposes its switch."""
import pytest

import cabi_header as hdr
import rot_mvgaze_amd  # noqa: F401

NEW_ENTRY_POINTS = ("mvg_conv_fprop_bf16_affine", "mvg_preprocess_u8hwc_resize_bf16")


@pytest.mark.parametrize("name", NEW_ENTRY_POINTS)
def test_new_entry_points_declared_bound_and_exported(name):
    assert name in hdr.functions, f"{name} is not declared in include/rotmvgaze.h"
    assert hdr.functions[name][0] == "int" and hdr.functions[name][1][-1] == ("void*", "stream")


def test_affine_signature_mirrors_the_fp32_one():
    """mvg_conv_fprop_bf16_affine(d, x, wgt, out, scale, shift, residual, relu, stream): the argument list of mvg_conv_fprop_affine."""
    names = hdr.parameter_names
    assert names("mvg_conv_fprop_bf16_affine") == names("mvg_conv_fprop_affine") == \
        ["d", "x", "wgt", "out", "scale", "shift", "residual", "relu", "stream"]
    assert names("mvg_preprocess_u8hwc_resize_bf16") == names("mvg_preprocess_u8hwc_resize")


def test_backbone_switch_and_debug_hook_defaults():
    from rot_mvgaze_amd.backbone import Backbone
    from rot_mvgaze_amd.model import MultiViewGaze
    m = MultiViewGaze(18, 3)
    bb = Backbone(18, dict(m.named_parameters(remove_duplicate=False)) | dict(m.named_buffers()))
    assert bb.bf16_fold_eval is True
    assert bb.split_eval is True
    assert Backbone._debug_units is None and bb._debug_units is None
