"""The host-only plan queries of the split conv kernels (mvg_conv_dgrad_split_stages, mvg_conv_wgrad_split_tile, next to
mvg_conv_fprop_split_stages): declared, bound, answering without a GPU - they launch nothing - and, for the shapes of
tests/test_split_forms_gpu.py, giving the forms those tests are there for (without a device the planners assume 256 CUs)."""

import pytest

import cabi_header as hdr
import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd import _lib, ops
from rot_mvgaze_amd._lib import ConvDesc

import test_split_forms_gpu as forms



@pytest.fixture()
def both_settings():
    cus = _lib.lib().mvg_device_cus()
    cus = cus if cus > 0 else 256
    try:
        yield (("all CUs", 0, 2), ("8 CUs", cus - 8, 1))
    finally:
        ops.set_reserved_cus(0)


def test_plan_queries_are_declared_and_have_signatures():
    for name, nargs in (("mvg_conv_dgrad_split_stages", 2), ("mvg_conv_wgrad_split_tile", 4)):
        assert name in hdr.functions, name + " is not declared in include/rotmvgaze.h"
        assert hdr.functions[name][0] == "int" and hdr.arity(name) == nargs


def test_plan_queries_reject_bad_descriptors():
    bad = ConvDesc.make(1, 2, 8, 8, 48, 64, 1, 1, 0)            # cin not a multiple of 32
    assert _lib.lib().mvg_conv_dgrad_split_stages(bad, 0) == -1
    assert _lib.lib().mvg_conv_wgrad_split_tile(bad, None, None, None) == -1
    with pytest.raises(RuntimeError, match="multiples of 32"):
        ops.conv_dgrad_split_stages(bad)
    with pytest.raises(RuntimeError, match="multiples of 32"):
        ops.conv_wgrad_split_tile(bad)
    ok = ConvDesc.make(1, 2, 8, 8, 64, 64, 1, 1, 0)
    assert _lib.lib().mvg_conv_wgrad_split_tile(ok, None, None, None) == 0         # every out-pointer may be NULL


def test_forward_and_backward_data_cases_get_both_k_loops(both_settings):
    for name, reserve, stages in both_settings:
        ops.set_reserved_cus(reserve)
        for c in forms.FPROP_CASES + forms.AFFINE_CASES:
            assert ops.conv_fprop_split_stages(forms.desc(forms.sq(*c))) == stages, (name, c)
        for c in forms.DGRAD_CASES:
            assert ops.conv_dgrad_split_stages(forms.desc(forms.sq(*c))) == stages, (name, c)
        for c in forms.BNREDUCE_CASES:
            assert ops.conv_dgrad_split_stages(forms.desc(forms.sq(*c)), True) == stages, (name, c)


def test_fused_reduce_counts_the_classes_without_taps(both_settings):
    # 1x1 stride 2: one parity class of four has a tap - 10 tiles without the reduce, 40 with it (30 of them epilogue only)
    d = forms.desc(forms.sq(2, 3, 28, 128, 256, 1, 2, 0))
    ops.set_reserved_cus(both_settings[1][1])
    assert ops.conv_dgrad_split_stages(d, False) == 2 and ops.conv_dgrad_split_stages(d, True) == 1
    # stride 1: one class either way
    d1 = forms.desc(forms.sq(2, 6, 14, 256, 256, 3, 1, 1))
    assert ops.conv_dgrad_split_stages(d1, False) == ops.conv_dgrad_split_stages(d1, True) == 1


def test_stage_queries_follow_the_plan_rule(both_settings):
    """<= 2 tiles per CU: pipelined; <= 4 per CU: pipelined with >= 48 K-steps; 64-column launches: single-stage always."""
    ops.set_reserved_cus(both_settings[1][1])                       # 8 CUs: thresholds 16 and 32 tiles
    def fwd(n, cin, cout):
        return ops.conv_fprop_split_stages(ConvDesc.make(1, n, 16, 16, cin, cout, 1, 1, 0))     # 2 n row tiles x cout / 128
    assert fwd(8, 64, 128) == 2 and fwd(9, 64, 128) == 1            # 16 / 18 tiles, 2 K-steps
    assert fwd(16, 1536, 128) == 2 and fwd(17, 1536, 128) == 1      # 32 / 34 tiles, 48 K-steps
    assert fwd(16, 1504, 128) == 1                                  # 32 tiles, 47 K-steps
    assert fwd(1, 64, 64) == 1                                      # 64 columns
    # backward-data plans on cin columns and cout K
    assert ops.conv_dgrad_split_stages(ConvDesc.make(1, 8, 16, 16, 128, 64, 1, 1, 0)) == 2
    assert ops.conv_dgrad_split_stages(ConvDesc.make(1, 9, 16, 16, 128, 64, 1, 1, 0)) == 1
    assert ops.conv_dgrad_split_stages(ConvDesc.make(1, 1, 16, 16, 64, 128, 1, 1, 0)) == 1


def test_wgrad_cases_get_their_tile_forms_and_cover_all_fourteen():
    got = [ops.conv_wgrad_split_tile(forms.desc(c)) for c in forms.WGRAD_CASES]
    assert got == forms.WGRAD_FORMS
    tiles = ((128, 256), (128, 192), (128, 128), (128, 64), (64, 192), (64, 128), (64, 64))
    assert set(got) == {(bm, bn, incr) for bm, bn in tiles for incr in (True, False)}
    for c, (bm, bn, incr) in zip(forms.WGRAD_CASES, got):
        d = forms.desc(c)
        assert incr == (d.ho * d.wo >= 32)
        assert bm == (128 if d.cout >= 128 else 64)


def test_wgrad_slab_counts_differ_where_the_gpu_test_says_so(both_settings):
    import ctypes as C
    for c in forms.WGRAD_SLABS_DIFFER:
        d, n = forms.desc(c), []
        for _, reserve, _ in both_settings:
            ops.set_reserved_cus(reserve)
            n.append(_lib.lib().mvg_conv_wgrad_splits_split(C.byref(d)))
        assert n[0] > n[1] >= 1, (c, n)
