"""The host-only plan queries of the bf16 conv kernels (mvg_conv_plan_query_bf16, mvg_conv_wgrad_tile_bf16): declared, bound,
rejecting what the launches reject, and giving every case of bf16_forms_ref's tables the form the table names - so that
tests/test_bf16_forms_gpu.py's guards can hold on a GPU - with per-class tiles and K-steps equal to the class table recomputed
from the descriptor.  And the GPU file's per-element bar for bf16 outputs is REACHABLE: fp32 arithmetic on the CPU (F.conv2d on the
same bf16-rounded operands, the epilogue in fp32, one rounding to bf16) stays inside it against float64 at every GEMM case.
No GPU."""
import ctypes as C

import pytest
import torch

import bf16_forms_ref as R
import cabi_header as hdr
import rot_mvgaze_amd  # noqa: F401

KINDS = ("MVG_PLAN_BF16_FPROP", "MVG_PLAN_BF16_DGRAD", "MVG_PLAN_BF16_DGRAD_BNREDUCE", "MVG_PLAN_BF16_AFFINE",
         "MVG_PLAN_BF16_LINEAR_FPROP_MIXED", "MVG_PLAN_BF16_LINEAR_DGRAD_MIXED")


def desc(case):
    from rot_mvgaze_amd._lib import ConvDesc
    return ConvDesc.make(*case)


def test_queries_are_declared_and_bound():
    from rot_mvgaze_amd import _lib
    for name, nargs in (("mvg_conv_plan_query_bf16", 3), ("mvg_conv_wgrad_tile_bf16", 5)):
        assert name in hdr.functions, name + " is not declared in include/rotmvgaze.h"
        assert hdr.functions[name][0] == "int" and hdr.arity(name) == nargs == len(_lib.SIGNATURES[name][1])
        assert hasattr(_lib.lib(), name)
    for k, name in enumerate(KINDS):
        assert hdr.constants[name] == k == getattr(_lib, name[4:])
    assert _lib.lib().mvg_abi_version() == _lib.ABI_VERSION == hdr.constants["MVG_ABI_VERSION"]


def test_queries_reject_what_the_launches_reject_and_tolerate_null_out_pointers():
    from rot_mvgaze_amd import _lib, ops
    L = _lib.lib()
    ok = desc((1, 2, 9, 9, 64, 64, 3, 1, 1))
    for kind in range(4):
        assert L.mvg_conv_plan_query_bf16(ok, kind, None) == 0
    assert L.mvg_conv_wgrad_tile_bf16(ok, 0, None, None, None) == 0 and L.mvg_conv_wgrad_tile_bf16(ok, 1, None, None, None) == 0
    lin = _lib.ConvDesc.linear(70, 72, 136)
    assert L.mvg_conv_plan_query_bf16(lin, _lib.PLAN_BF16_LINEAR_FPROP_MIXED, None) == 0
    assert L.mvg_conv_plan_query_bf16(lin, _lib.PLAN_BF16_LINEAR_DGRAD_MIXED, None) == 0
    bad = [desc((1, 2, 9, 9, 12, 64, 1, 1, 0)),          # cin % 8
           desc((1, 2, 9, 9, 64, 12, 1, 1, 0)),          # cout % 8
           desc((1, 2, 9, 9, 96, 64, 3, 1, 1)),          # a 3x3 needs power-of-two channels
           desc((1, 2, 9, 9, 64, 64, 3, 3, 1))]          # stride 3
    for d in bad:
        for kind in range(6):
            assert L.mvg_conv_plan_query_bf16(d, kind, None) == -1
        assert L.mvg_conv_wgrad_tile_bf16(d, 0, None, None, None) == -1
    assert L.mvg_conv_plan_query_bf16(None, 0, None) == -1 and L.mvg_conv_wgrad_tile_bf16(None, 0, None, None, None) == -1
    assert L.mvg_conv_plan_query_bf16(ok, 6, None) == -1 and L.mvg_conv_plan_query_bf16(ok, -1, None) == -1      # unknown kind
    with pytest.raises(RuntimeError, match="unknown kind"):
        ops.conv_plan_query_bf16(ok, 9)
    with pytest.raises(RuntimeError, match="multiples of 8"):
        ops.conv_wgrad_tile_bf16(bad[0])
    # the fused reduce takes the uniform-tap kernel only: 32 channels per tap are the plain backward-data launch's
    narrow = desc((1, 2, 9, 9, 64, 32, 1, 1, 0))
    assert L.mvg_conv_plan_query_bf16(narrow, _lib.PLAN_BF16_DGRAD, None) == 0
    with pytest.raises(RuntimeError, match="multiples of 64"):
        ops.conv_plan_query_bf16(narrow, _lib.PLAN_BF16_DGRAD_BNREDUCE)
    # backward-data on fp32 operands: stride 1 only
    with pytest.raises(RuntimeError, match="stride 1"):
        ops.conv_plan_query_bf16(desc((1, 2, 9, 9, 64, 64, 1, 2, 0)), _lib.PLAN_BF16_LINEAR_DGRAD_MIXED)
    # the out structure is written only on success
    pl = _lib.ConvPlan(bm=-7)
    assert L.mvg_conv_plan_query_bf16(bad[0], 0, C.byref(pl)) == -1 and pl.bm == -7


def _plan_matches(pl, want, what):
    kernel, bn, fasta, tiles, kt = want
    assert (pl["bm"], pl["bk"], pl["streamk_grid"], pl["splitk"], pl["scratch_floats"]) == (128, 64, 0, 1, 0), what
    assert (pl["bn"], pl["fasta"], pl["cls_tiles"], pl["cls_kt"]) == (bn, fasta, tiles, kt), f"{what}: {pl}"


def test_every_table_case_gets_the_form_the_table_names():
    from rot_mvgaze_amd import _lib, ops
    seen = set()
    for case, fwd, bwd in R.GEMM_CASES:
        for dgrad, form, kind, tag in ((False, fwd, _lib.PLAN_BF16_FPROP, "fwd"), (True, bwd, _lib.PLAN_BF16_DGRAD, "bwd")):
            if form is None:
                continue
            pl, want = ops.conv_plan_query_bf16(desc(case), kind), R.gemm_plan(case, dgrad)
            assert want[:2] == form, f"{case} {tag}: the restated rule gives {want[:2]}, the table {form}"
            _plan_matches(pl, want, f"{case} {tag}")
            assert pl["kernel"] == form[0]
            seen.add((tag, pl["kernel"], pl["bn"]))
    for case, form in R.AFFINE_CASES:
        pl, want = ops.conv_plan_query_bf16(desc(case), _lib.PLAN_BF16_AFFINE), R.gemm_plan(case, False)
        assert want[:2] == form
        _plan_matches(pl, want, f"{case} affine")
        assert pl == ops.conv_plan_query_bf16(desc(case), _lib.PLAN_BF16_FPROP), "the affine kernels follow the training forward's choice"
        seen.add(("affine", pl["kernel"], pl["bn"]))
    for rc, bn in R.REDUCE_CASES:
        case = R.reduce_case(rc)
        pl, want = ops.conv_plan_query_bf16(desc(case), _lib.PLAN_BF16_DGRAD_BNREDUCE), R.gemm_plan(case, True, True)
        assert want[:2] == (R.DMA, bn)
        _plan_matches(pl, want, f"{rc} fused reduce")
        seen.add(("bnreduce", pl["kernel"], pl["bn"]))
    assert ops.conv_plan_query_bf16(desc(R.reduce_case(R.REDUCE_CASES[2][0])), _lib.PLAN_BF16_DGRAD_BNREDUCE)["cls_kt"] == [1, 0, 0, 0]
    for (rows, fin, fout), fwd, bwd in R.LINEAR_CASES:
        d, case = _lib.ConvDesc.linear(rows, fin, fout), R.linear_case(rows, fin, fout)
        for dgrad, form, kind, tag in ((False, fwd, _lib.PLAN_BF16_LINEAR_FPROP_MIXED, "lin_fwd"),
                                       (True, bwd, _lib.PLAN_BF16_LINEAR_DGRAD_MIXED, "lin_bwd")):
            pl, want = ops.conv_plan_query_bf16(d, kind), R.gemm_plan(case, dgrad)
            assert (want[2], want[1]) == form
            _plan_matches(pl, want, f"{(rows, fin, fout)} {tag}")
            assert pl["kernel"] == "mixed"
            seen.add((tag, pl["fasta"], pl["bn"]))
    for case, tile in R.WGRAD_CASES:
        assert ops.conv_wgrad_tile_bf16(desc(case)) == tile == R.wgrad_tile(case), case
        assert ops.conv_wgrad_tile_bf16(desc(case), True) == tile[:2] + (False,)
        seen.add(("wgrad",) + tile)
    for (rows, fin, fout), tile in R.MIXED_WGRAD_CASES:
        got = ops.conv_wgrad_tile_bf16(_lib.ConvDesc.linear(rows, fin, fout), True)
        assert got == tile + (False,) == R.wgrad_tile(R.linear_case(rows, fin, fout), True)
        seen.add(("wgrad_mixed",) + got)
    assert seen == R.FORMS == R.table_forms(), (sorted(R.FORMS - seen, key=str), sorted(seen - R.FORMS, key=str))


def test_table_cases_reach_the_edges_they_are_listed_for():
    """The properties the GPU cases are there for, recomputed from the descriptors."""
    from igemm_forms_ref import class_table, out_hw
    rows = lambda case, dgrad: [r for r, _, _ in class_table(case, dgrad)]
    assert rows(R.GEMM_CASES[0][0], False) == [162] and 162 % 128 == 34                 # a last tile whose second wave row is empty
    assert [t for _, t, _ in class_table((1, 1, 10, 10, 64, 64, 7, 2, 3), True)] == [16, 12, 12, 9]
    assert [t for _, t, _ in class_table((1, 2, 12, 12, 8, 64, 7, 2, 3), True)] == [16, 12, 12, 9]
    assert [t for _, t, _ in class_table((2, 2, 9, 7, 64, 64, 3, 2, 1), True)] == [4, 2, 2, 1]
    assert len(class_table((1, 2, 9, 9, 64, 64, 1, 2, 0), True)) == 1 and len(R.kept_class_table((1, 2, 9, 9, 64, 64, 1, 2, 0))) == 4
    assert R.gemm_plan((1, 2, 7, 7, 64, 64, 5, 1, 2), False)[4] == [25] and R.gemm_plan((1, 1, 10, 10, 128, 64, 7, 2, 3), False)[4] == [98]
    for case, _ in R.WGRAD_CASES:                                                        # splits that start mid-image, trailing empty ones
        G, N, h, w, cin, cout, k, st, pad = case
        ho, wo = out_hw(case)
        one, three, many = R.wgrad_split_counts(case)
        assert (one, three) == (1, 3) and (many - 3) * 64 >= G * N * ho * wo > (many - 4) * 64
    assert any((-(-G * N * out_hw(c)[0] * out_hw(c)[1] // 3) + 63) // 64 * 64 % (out_hw(c)[0] * out_hw(c)[1]) != 0
               for c, _ in R.WGRAD_CASES for G, N in [c[:2]])
    assert sorted(s for _, s in R.WGRAD_DEFER_CASES) == [3, 9, 33]                      # below 8, 8 .. 31, from 32: 1, 4, 16 lanes


def _held(got32, ref64, magnitude, what):
    ratio = R.bound_ratio(R.q(got32), ref64, magnitude)
    assert ratio <= 1.0, f"{what}: fp32 arithmetic rounded once to bf16 is at {ratio:.3f} of the bar"
    return ratio


@pytest.mark.parametrize("case,fwd,bwd", R.GEMM_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) and len(v) == 9 else None)
def test_the_bf16_bar_is_reachable_by_fp32_arithmetic_rounded_once(case, fwd, bwd):
    """Nothing here runs the library: the bar of the GPU file must not ask more than fp32 accumulation and ONE rounding give."""
    p = R.gemm_problem(case)
    y32, dx32, _ = p.conv(torch.float32)
    worst = 0.0
    if fwd is not None:
        worst = max(worst, _held(y32, p.y64, p.y64.abs().max(), f"{case} y"))
        scale, shift, res = R.affine_operands(case[5], tuple(p.y64.shape))
        for with_res in (False, True):
            for relu in (False, True):
                o32, o64 = y32 * scale + shift, p.y64 * scale.double() + shift.double()
                mag = (p.y64 * scale.double()).abs() + shift.double().abs()
                if with_res:
                    o32, o64, mag = o32 + res, o64 + res.double(), mag + res.double().abs()
                if relu:
                    o32, o64 = torch.relu(o32), torch.relu(o64)
                worst = max(worst, _held(o32, o64, mag.max(), f"{case} affine residual={with_res} relu={relu}"))
    if bwd is not None:
        worst = max(worst, _held(dx32, p.dx64, p.dx64.abs().max(), f"{case} dx"))
        a = p.addend
        worst = max(worst, _held(dx32 + a, p.dx64 + a.double(), (p.dx64.abs() + a.double().abs()).max(), f"{case} dx + addend"))
    print(f"BF16-FORMS-CPU {case}: largest bound ratio {worst:.3f}")


def test_the_bf16_bar_rejects_a_truncating_store():
    """... and it is a bar: the same fp32 values truncated to bf16 instead of rounded miss it on a large share of the elements,
    where the max-norm bar of test_bf16_gpu.py (OUT_RTOL = 6e-3 of max |ref|) accepts them."""
    p = R.gemm_problem(R.GEMM_CASES[0][0])
    y32 = p.conv(torch.float32)[0].contiguous()
    trunc = (y32.view(torch.int32) & ~0xFFFF).view(torch.float32)
    bound = R.bf16_bound(p.y64, p.y64.abs().max())
    miss = ((trunc.double() - p.y64).abs() > bound).double().mean().item()
    assert miss > 0.1, miss
    assert (trunc.double() - p.y64).abs().max() <= 6e-3 * p.y64.abs().max()
