"""The case tables, references and derived bars of tests/fusion_split_forms_ref.py checked on their own (no GPU), and the host-only
plan query mvg_linear_plan_query_split: declared, bound, launching nothing, refusing what the launches refuse and - without a device
the planners assume 256 CUs - giving every Linear case of tests/test_fusion_split_forms_gpu.py the instantiation its table row names
under each of the three settings.  The bars of the GPU file are derived, not measured: here the kernels' sums restated in numpy
float32 on the case inputs stay inside them, so they can be met."""
import ctypes as C

import numpy as np
import pytest
import torch

import cabi_header as hdr
import rot_mvgaze_amd  # noqa: F401
import fusion_split_forms_ref as R
from rot_mvgaze_amd import _lib, ops
from rot_mvgaze_amd._lib import ConvDesc


@pytest.fixture()
def three_settings():
    cus = _lib.lib().mvg_device_cus()
    cus = cus if cus > 0 else R.DEVICE_CUS
    assert cus == R.DEVICE_CUS, f"the case tables are written for a {R.DEVICE_CUS}-CU device"
    try:
        yield R.settings(cus)
    finally:
        ops.set_reserved_cus(0)


def test_linear_plan_query_is_declared_bound_and_launches_nothing():
    name = "mvg_linear_plan_query_split"
    assert name in hdr.functions and hdr.functions[name][0] == "int" and hdr.arity(name) == 7
    assert len(_lib.SIGNATURES[name][1]) == 7
    L = _lib.lib()
    assert L.mvg_linear_plan_query_split(300, 64, 800, 0, None, None, None) == 0          # every out-pointer may be NULL
    assert L.mvg_linear_plan_query_split(300, 64, 800, 1, None, None, None) == 0
    assert ops.linear_plan_query_split(300, 64, 800)[0] == 128 and ops.linear_plan_query_split(300, 800, 64, dgrad=True)[0] == 128


@pytest.mark.parametrize("sizes", [(300, 48, 800), (300, 64, 808), (300, 64, 16), (0, 64, 128)])
def test_linear_plan_query_refuses_what_the_launches_refuse(sizes):
    L = _lib.lib()
    rows, fin, fout = sizes
    for dgrad in (0, 1):
        bm = C.c_int32(-7)
        assert L.mvg_linear_plan_query_split(rows, fin, fout, dgrad, C.byref(bm), None, None) == -1 and bm.value == -7
        assert L.mvg_last_error()
    if sizes[0] > 0:
        with pytest.raises(RuntimeError, match="multiples of 32"):
            ops.linear_plan_query_split(*sizes)


def test_every_linear_case_gets_the_form_its_row_names(three_settings):
    for shape, forms, _ in R.LINEAR_CASES:
        rows, fin, fout = shape
        assert max(rows * fin, rows * fout, fin * fout) <= 1100 * 1536, "no operand larger than 1100 x 1536"
        for (name, reserve), (bn, stages), (_, keep) in zip(three_settings, forms, R.SETTING_CUS):
            ops.set_reserved_cus(reserve)
            assert ops.linear_plan_query_split(rows, fin, fout) == (128, bn, stages), (shape, name)
            assert ops.linear_plan_query_split(rows, fout, fin, dgrad=True) == (128, bn, stages), (shape, name, "backward-data")
            assert R.linear_plan(rows, fin, fout, False, keep or R.DEVICE_CUS) == (bn, stages), (shape, name, "the rule restated")
            assert R.linear_plan(rows, fout, fin, True, keep or R.DEVICE_CUS) == (bn, stages)


def test_the_plan_is_the_linears_own_not_the_convs(three_settings):
    """The same descriptor planned as a conv (lin = false) keeps 128 columns and has no two-stage loop at 64 columns."""
    ops.set_reserved_cus(three_settings[0][1])
    assert ops.linear_plan_query_split(300, 64, 800) == (128, 64, 2)
    assert ops.linear_plan_query_split(1100, 96, 96) == (128, 64, 2)
    assert ops.conv_fprop_split_stages(ConvDesc.linear(1100, 96, 96)) == 1           # the convs' rule: 64 columns run single-stage
    assert ops.conv_dgrad_split_stages(ConvDesc.linear(1100, 96, 96)) == 1


def test_the_long_k_boundary(three_settings):
    long_k, short_k = R.LONG_K_BOUNDARY
    ops.set_reserved_cus(three_settings[2][1])                      # 8 CUs: 21 tiles lie between 2 and 4 per CU
    assert ops.linear_plan_query_split(*long_k) == (128, 128, 2) and ops.linear_plan_query_split(*short_k) == (128, 128, 1)
    m = lambda s: (s[0], s[2], s[1])
    assert ops.linear_plan_query_split(*m(long_k), dgrad=True) == (128, 128, 2)
    assert ops.linear_plan_query_split(*m(short_k), dgrad=True) == (128, 128, 1)
    assert long_k[1] // 32 == 48 and short_k[1] // 32 == 47


def test_the_tables_cover_every_form():
    assert R.table_forms() == R.FORMS
    assert len([f for f in R.FORMS if f[0] == "linear"]) == 8 and len([f for f in R.FORMS if f[0] == "wgrad"]) == 7
    # same column tile, both K loops, in one row: what the across-settings equality of the GPU file rests on
    for want in ((128, {1, 2}), (64, {1, 2})):
        assert any({st for bn, st in forms if bn == want[0]} == want[1] for _, forms, _ in R.LINEAR_CASES), want
    ksteps = {-(-fin // 32) for (rows, fin, fout), forms, _ in R.LINEAR_CASES if (64, 2) in forms}
    assert {1, 2, 3} <= ksteps
    ksteps128 = {(-(-fin // 32), st) for (rows, fin, fout), forms, _ in R.LINEAR_CASES for bn, st in forms if bn == 128}
    assert {(1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (3, 2)} <= ksteps128
    assert {1, 127, 129} <= {rows for (rows, fin, fout), _, _ in R.LINEAR_CASES}


def test_every_weight_gradient_case_gets_its_tile(three_settings):
    slabs_differ = 0
    for shape, tile, differ in R.WGRAD_CASES:
        rows, fin, fout = shape
        d = ConvDesc.linear(rows, fin, fout)
        assert ops.conv_wgrad_split_tile(d) == tile + (False,), shape               # ho * wo = 1 < 32: never the incremental form
        assert R.wgrad_tile(rows, fin, fout) == tile
        assert rows in (1, 200, 1100) and max(rows * fin, rows * fout, fin * fout) <= 1100 * 1536
        n = []
        for _, reserve in (three_settings[0], three_settings[2]):
            ops.set_reserved_cus(reserve)
            n.append(_lib.lib().mvg_conv_wgrad_splits_split(C.byref(d)))
        assert min(n) >= 1 and (n[0] > n[1]) == differ, (shape, n)
        slabs_differ += differ
    assert slabs_differ >= 2 and {t for _, t, _ in R.WGRAD_CASES} == set(R.TILES)
    assert any(-(-rows // 16) * 16 != rows for (rows, _, _), _, _ in R.WGRAD_CASES), "a ragged last K-step of 16 rows"


def test_bound_derived_scales_keep_the_sp_results_inside_fp16_and_agree_with_elem_h():
    import test_prep_forms_cpu as P
    P.test_sp_scale_for_matches_elem_h()                           # sp_scale_for against elem.h's function, its constants included
    for shape, _, _ in R.LINEAR_CASES:
        rows, fin, fout = shape
        inp = R.linear_inputs(rows, fin, fout)
        x_sinv, w_sinv = 1.0 / R.scale_of(inp.x), 1.0 / R.scale_of(inp.w)
        y = torch.relu(inp.x.double() @ inp.w.double().t() + inp.b.double())
        for bias_am in (float(inp.b.abs().max()), 0.0):
            bound, sinv = R.lin_out_sinv(fin, x_sinv, w_sinv, bias_am)
            s = 1.0 / float(sinv)
            assert np.log2(s) == round(np.log2(s)) and 2.0 ** 14 <= float(bound) * s < 2.0 ** 15, shape
            # the bound is a bound: |x| < 2^15 x_sinv, |w| < 2^15 w_sinv, fin products (+ the bias where its abs-max is given)
            assert float(y.max()) * s < 2.0 ** 15, (shape, bias_am)
            exact = fin * 2.0 ** 30 * x_sinv * w_sinv + float(np.float32(bias_am))      # one fp32 rounding: the addition's
            assert abs(float(bound) - exact) <= R.U * exact


@pytest.mark.parametrize("cols", R.COLSUM_COLS)
@pytest.mark.parametrize("rows", R.COLSUM_ROWS)
def test_split_colsum_bar_is_reachable(rows, cols):
    for mag in R.COLSUM_MAGS + (0.0,):
        g, db0 = R.colsum_inputs(rows, cols, mag)
        assert bool((db0 != 0).all())
        col = g.double().sum(0)
        for start in (None, db0):
            err = (torch.from_numpy(R.colsum_f32(g, start)).double() - (col + (start.double() if start is not None else 0.0))).abs()
            assert bool((err <= R.colsum_bound(g, start)).all()), (rows, cols, mag, start is not None)
        # the host pieces of the scaled gradient compare clean against themselves: the exception share at 0
        scale = R.sp_scale_for(float(g.abs().max()))
        stored = g.numpy() * np.float32(scale)
        assert R.sp_compare(R.sp_pieces(stored), stored) == (0, 0, 0.0)
        assert mag == 0.0 or 2.0 ** 14 <= float(np.abs(stored).max()) < 2.0 ** 15


@pytest.mark.parametrize("size", R.BUILD_SIZES, ids=lambda s: f"cf{s[0]}_nvec{s[1]}")
def test_fuse_build_bars_are_reachable(size):
    cf, nvec, mag = size
    pb = R.build_inputs(cf, nvec, mag)
    assert pb.rows == 30 and cf % 8 == 0 and nvec % 8 == 0
    want, absterms = pb.rotated(True)
    o = pb.rotated_f32()
    # the three-term expression alone: inside 3 u sum |r f|
    assert bool(((torch.from_numpy(o).double() - want).abs() <= 3 * R.U * absterms).all())
    # ... and stored in sp times the kernel's scale, read back: inside the whole bar with no element excused
    stored = o * np.float32(pb.sf)
    assert float(np.abs(stored).max()) < 2.0 ** 15, "|rel @ f| <= sqrt(3) max |f|: the scale's bound"
    back = torch.from_numpy(R.sp_merge(R.sp_pieces(stored)).astype(np.float64) / pb.sf)
    assert bool(((back - want).abs() <= R.build_bound(want, absterms, 1.0 / pb.sf)).all())
    # without a rotation the expression is a copy
    ident, _ = pb.rotated(False)
    assert torch.equal(ident, pb.F.double()[pb.partner.long()])
    for scale, top in ((pb.sf, max(pb.am_img, R.SQRT3_F32 * pb.am_feat)), (pb.sh, max(pb.am_img, pb.am_feat))):
        assert 2.0 ** 14 <= float(top) * scale < 2.0 ** 15


def test_fuse_build_sizes_pass_256_chunks_in_both_loops():
    assert any(cf // 8 > 256 for cf, _, _ in R.BUILD_SIZES) and any(3 * nvec // 8 > 256 for _, nvec, _ in R.BUILD_SIZES)


@pytest.mark.parametrize("case", R.unbuild_cases(), ids=str)
def test_fuse_unbuild_bars_are_reachable(case):
    uc = R.UnbuildCase(*case)
    dF, da = uc.f32()
    assert bool(((torch.from_numpy(dF).double() - uc.dF).abs() <= uc.dF_bound).all())
    assert bool(((torch.from_numpy(da).double() - uc.da).abs() <= uc.da_bound).all())
    assert uc.dF.abs().max() > 0 and uc.da.abs().max() > 0


def test_fuse_unbuild_cases_cover_the_issue_list():
    cases = R.unbuild_cases()
    assert {c[4] for c in cases} == set(R.UNBUILD_MODES) and {c[5] for c in cases} == {True, False} == {c[6] for c in cases}
    assert {(c[0], c[1]) for c in cases} == set(R.UNBUILD_VB) and {(c[2], c[3]) for c in cases} == set(R.UNBUILD_SIZES)
    assert (6 * 5) % 4 != 0, "V = 3, B = 5: the last workgroup of four feature rows holds two"
    assert any(cf // 4 > 256 and nvec > 256 for cf, nvec in R.UNBUILD_SIZES)


def test_absmax_tensors_are_the_issue_list():
    vs = R.absmax_tensors()
    c = R.ABSMAX_COUNTS
    assert c[:5] == (0, 1, 255, 257, 300001) and R.ABSMAX_GRID < c[5] <= 1100 * 1536 and len(vs) == 8
    assert float(vs[4][0]) == float(vs[4][:c[4]].abs().max()) and float(vs[5][c[5] - 1]) == -float(vs[5][:c[5]].abs().max())
    assert not vs[6].any() and all(v.numel() >= max(n, 1) for v, n in zip(vs, c))
