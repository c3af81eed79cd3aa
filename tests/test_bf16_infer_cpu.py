"""CPU-side checks of the bf16 inference path's boundary: the header declares the new entry points, the binding
lists them with the header's arity, the library exports them, and the backbone exposes its switch."""
import os
import re

import pytest

import rot_mvgaze_amd  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("mvg_conv_fprop_bf16_affine", "mvg_preprocess_u8hwc_resize_bf16")


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from rot_mvgaze_amd import _lib
    return _lib.lib()


def _header_args(name):
    hdr = open(os.path.join(ROOT, "include", "rotmvgaze.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/rotmvgaze.h"
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", NEW_ENTRY_POINTS)
def test_new_entry_points_declared_bound_and_exported(built_lib, name):
    from rot_mvgaze_amd import _lib
    args = _header_args(name)
    assert name in _lib.SIGNATURES, f"{name} missing from _lib.SIGNATURES"
    res, argtypes = _lib.SIGNATURES[name]
    assert len(argtypes) == len(args), (name, len(argtypes), args)
    assert hasattr(built_lib, name)
    assert args[-1].replace(" ", "") == "void*stream"


def test_affine_signature_mirrors_the_fp32_one():
    """mvg_conv_fprop_bf16_affine(d, x, wgt, out, scale, shift, residual, relu, stream): the argument list of mvg_conv_fprop_affine."""
    names = lambda args: [re.sub(r".*[\s\*]", "", a) for a in args]
    assert names(_header_args("mvg_conv_fprop_bf16_affine")) == names(_header_args("mvg_conv_fprop_affine")) == \
        ["d", "x", "wgt", "out", "scale", "shift", "residual", "relu", "stream"]
    assert names(_header_args("mvg_preprocess_u8hwc_resize_bf16")) == names(_header_args("mvg_preprocess_u8hwc_resize"))


def test_abi_version_in_header_binding_and_library_agree(built_lib):
    from rot_mvgaze_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rotmvgaze.h")).read()
    assert re.search(r"#define\s+MVG_ABI_VERSION\s+13\b", hdr)
    assert _lib.ABI_VERSION == 13 == built_lib.mvg_abi_version()


def test_backbone_switch_and_debug_hook_defaults():
    from rot_mvgaze_amd.backbone import Backbone
    from rot_mvgaze_amd.model import MultiViewGaze
    m = MultiViewGaze(18, 3)
    bb = Backbone(18, dict(m.named_parameters(remove_duplicate=False)) | dict(m.named_buffers()))
    assert bb.bf16_fold_eval is True
    assert bb.split_eval is True
    assert Backbone._debug_units is None and bb._debug_units is None
