"""No GPU: (1) the float64 restatements of tests/bn_forms_ref.py against PyTorch's own BatchNorm on CPU - partial writer ->
merge must reproduce F.batch_norm's batch statistics and running-statistics updates, the backward formulas autograd; (2) the
host-only plan query of the BatchNorm passes (mvg_bn_plan_query): declared, its plan's fields the keys ops.bn_plan_query returns, and - without a device the planners
assume 256 CUs - the tabulated form for every case of tests/test_bn_forms_gpu.py, the launches' rejection messages, and a
workspace (mvg_bn_bwd_workspace_floats / mvg_bn_eval_bwd_workspace_floats) that holds what the reported chunks write."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import cabi_header as hdr
import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd import _lib, ops
from rot_mvgaze_amd._lib import (BN_PASS_APPLY, BN_PASS_BWD_APPLY, BN_PASS_BWD_REDUCE, BN_PASS_EVAL_BWD, BN_PASS_FINALIZE,
                                 BN_PASS_POOL_BWD_REDUCE, BN_PASS_POOL_EVAL_BWD, BnPlan)

import bn_forms_ref as ref
from bn_forms_ref import BF16, EPS, FP32, MOMENTUM, SP



@pytest.fixture()
def reserve():
    """reserve(n): leave n CUs to the planners (0: all); reset afterwards."""
    cus = _lib.lib().mvg_device_cus()
    cus = cus if cus > 0 else 256
    try:
        yield lambda n: ops.set_reserved_cus(cus - n if n else 0)
    finally:
        ops.set_reserved_cus(0)


# ---------------------------------------------------------------- the restatement itself
@pytest.mark.parametrize("G,rows,C,rpp,slots", [(1, 640, 8, 64, None), (3, 64 * 7 - 17, 5, 64, None), (2, 200, 4, 32, 11), (2, 65, 3, 64, 4),
                                                (1, 1, 4, 64, 2)])
def test_partial_writer_and_merge_reproduce_batch_norm_statistics(G, rows, C, rpp, slots):
    x = ref.randn((G, rows, C), rows + C) * 1.7 + ref.randn((1, 1, C), 3)
    gamma, beta = ref.randn((C,), 4) * 0.2 + 1, ref.randn((C,), 5)
    rm0, rv0 = ref.randn((C,), 6), ref.randn((C,), 7).abs() + 0.5
    stats = ref.write_partials(x, rpp, slots)
    valid = -(-rows // rpp)
    assert stats.shape == (G, slots or valid, 2, C) and bool(torch.isfinite(stats[:, :valid]).all())
    assert bool(torch.isnan(stats[:, valid:]).all())
    got = ref.merge_partials(stats, rows, rpp, gamma, beta, rm0, rv0)
    rm, rv = rm0.double().clone(), rv0.double().clone()
    for g in range(G):
        xg = x[g].double().t().reshape(1, C, rows)             # (N, C, L)
        if rows > 1:
            out = F.batch_norm(xg, rm, rv, gamma.double(), beta.double(), True, MOMENTUM, EPS)      # updates rm, rv in place
            want = x[g].double() * got["scale"][g] + got["shift"][g]
            assert float((out[0].t() - want).abs().max()) <= 2e-6 * float(out.abs().max())          # the partials are fp32
        else:                                                   # F.batch_norm refuses one value per channel: by hand
            rm = (1 - MOMENTUM) * rm + MOMENTUM * xg[0, :, 0]
            rv = (1 - MOMENTUM) * rv + MOMENTUM * 0.0
        mean, var = xg.mean((0, 2)), xg.var((0, 2), unbiased=False)
        # the sums were rounded to fp32 once per partial: relative 2^-24 of sums of like-signed terms, and margin
        assert float((got["mean"][g] - mean).abs().max()) <= 1e-6 * float(xg.abs().max())
        assert float((got["invstd"][g] - 1 / torch.sqrt(var + EPS)).abs().max()) <= 1e-5 * float((1 / torch.sqrt(var + EPS)).max())
    # the running statistics: fp32 recurrence against F.batch_norm's float64 one
    assert float((got["rm"].double() - rm).abs().max()) <= 1e-6 * max(float(rm.abs().max()), 1.0)
    assert float((got["rv"].double() - rv).abs().max()) <= 1e-6 * max(float(rv.abs().max()), 1.0)
    none = ref.merge_partials(stats, rows, rpp, gamma, beta)
    assert none["rm"] is None and none["rv"] is None and torch.equal(none["mean"], got["mean"])


def test_merge_clamps_a_constant_channel_and_counts_the_ragged_partial():
    x = torch.full((1, 100, 2), 0.1)
    x[0, :, 1] = torch.arange(100, dtype=torch.float32)
    got = ref.merge_partials(ref.write_partials(x, 64), 100, 64, torch.ones(2), torch.zeros(2))
    assert abs(float(got["invstd"][0, 0]) - EPS ** -0.5) <= 1e-3 and float(got["unbiased"][0, 0]) < 1e-12
    assert abs(float(got["mean"][0, 1]) - 49.5) < 1e-9 and abs(float(got["unbiased"][0, 1]) - 100 * 101 / 12) < 1e-6
    # ... and a wrong count for the ragged partial is not the same number (what the kernel's correction term is for)
    st = ref.write_partials(x, 64)
    assert abs(float(ref.merge_partials(st, 128, 64, torch.ones(2), torch.zeros(2))["mean"][0, 1]) - 49.5) > 1


@pytest.mark.parametrize("relu,res", [(True, True), (False, False), (True, False)])
def test_backward_formulas_are_autograd_of_batch_norm(relu, res):
    G, rows, C = 2, 50, 6
    y, go = ref.randn((G, rows, C), 1) * 2 + 0.5, ref.randn((G, rows, C), 2)
    r = ref.randn((G, rows, C), 3) if res else None
    gamma, beta = ref.randn((C,), 4) * 0.2 + 1, ref.randn((C,), 5) * 0.2
    yr, gr, br = y.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rr = r.double().requires_grad_(True) if res else None
    pre = torch.stack([F.batch_norm(yr[g].t()[None], None, None, gr, br, True, MOMENTUM, EPS)[0].t() for g in range(G)])
    pre = pre + rr if res else pre
    out = F.relu(pre) if relu else pre
    out.backward(go.double())
    mean, invstd = ref.group_stats(y)
    scale = gamma.double()[None] * invstd
    p2, o2 = ref.apply_ref(y, scale, beta.double()[None] - mean * scale, r, None, relu)
    assert float((o2 - out.detach()).abs().max()) <= 1e-12 * float(out.detach().abs().max())
    b = ref.train_bwd_ref(go, y, mean, invstd, gamma, (p2 > 0) if relu else None)
    for name, want in (("dy", yr.grad), ("dgamma", gr.grad), ("dbeta", br.grad)):
        assert float((b[name] - want).abs().max()) <= 1e-11 * float(want.abs().max()), name
    if res:
        assert float((b["dz"] - rr.grad).abs().max()) <= 1e-12
    # eval mode: the running statistics, no batch coupling
    rm, rv = ref.randn((C,), 8), ref.randn((C,), 9).abs() + 0.5
    yr, gr, br = y.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    pre = torch.stack([F.batch_norm(yr[g].t()[None], rm.double(), rv.double(), gr, br, False, MOMENTUM, EPS)[0].t() for g in range(G)])
    (F.relu(pre) if relu else pre).backward(go.double())
    e = ref.eval_bwd_ref(go, y, gamma, rm, rv, EPS, (pre.detach() > 0) if relu else None)
    for name, want in (("dy", yr.grad), ("dgamma", gr.grad), ("dbeta", br.grad)):
        assert float((e[name] - want).abs().max()) <= 1e-11 * float(want.abs().max()), name


def test_mask_bytes_and_dy_scale():
    on = torch.tensor([1, 0, 0, 1, 0, 0, 0, 0, 1, 1, 1, 1, 0, 1, 0, 0], dtype=torch.bool)
    assert ref.mask_bytes(on, 4).tolist() == [9, 0, 15, 2] and ref.mask_bytes(on, 8).tolist() == [9, 47]
    one = torch.ones(1, 1)
    sinv, m = ref.dy_scale_inverse(torch.ones(1), one, 0 * one, 0 * one, 3 * one, 10)      # bound 3 = 0.75 * 2^2: k = 13
    assert sinv == 2.0 ** -13 and m == 0.75


# ---------------------------------------------------------------- the query
def test_bn_plan_query_is_declared_and_bound():
    assert hdr.functions["mvg_bn_plan_query"][0] == "int" and hdr.arity("mvg_bn_plan_query") == 11
    (_, elem, G, rows, Cc), _ = next(iter(ref.STREAM_CASES.items()))
    assert hdr.field_names("mvg_bn_plan") == list(ops.bn_plan_query(BN_PASS_APPLY, elem, G, rows, Cc))
    assert C.sizeof(BnPlan) == 8 + 9 * 4 + 4 + 2 * 8 + 4 * 4 + 8
    for group, prefix in ((("APPLY", "BWD_APPLY", "BWD_REDUCE", "EVAL_BWD", "POOL_BWD_REDUCE", "POOL_EVAL_BWD", "FINALIZE"), "BN_PASS_"),
                          (("FP32", "BF16", "SP"), "BN_ELEM_"), (("WALK_GROUPS", "ALL_GROUPS", "PER_GROUP"), "BN_MERGE_")):
        for k, name in enumerate(group):
            assert hdr.constants["MVG_" + prefix + name] == getattr(_lib, prefix + name) == k
    assert (ref.FP32, ref.BF16, ref.SP) == (_lib.BN_ELEM_FP32, _lib.BN_ELEM_BF16, _lib.BN_ELEM_SP)
    assert (ref.WALK_GROUPS, ref.ALL_GROUPS, ref.PER_GROUP) == (_lib.BN_MERGE_WALK_GROUPS, _lib.BN_MERGE_ALL_GROUPS, _lib.BN_MERGE_PER_GROUP)


def test_streaming_cases_have_the_tabulated_form():
    for (name, elem, G, rows, Cc), want in ref.STREAM_CASES.items():
        for p in (BN_PASS_APPLY, BN_PASS_BWD_APPLY):
            pl = ops.bn_plan_query(p, elem, G, rows, Cc)
            assert (pl["accesses_per_group"], pl["grid_x"], pl["trips"], pl["step"]) == want, (name, elem, pl)
            assert pl["chunks"] == 0 and pl["lanes_per_group"] == 0
    # the second trip needs more than 2^20 accesses per group; the largest kernel-level case before these had 100 352
    assert ops.bn_plan_query(BN_PASS_APPLY, FP32, 2, 2 * 56 * 56, 64)["trips"] == 1
    assert ops.bn_plan_query(BN_PASS_APPLY, FP32, 1, 65536, 64)["trips"] == 1 and ops.bn_plan_query(BN_PASS_APPLY, FP32, 1, 65537, 64)["trips"] == 2


def test_reduce_cases_have_the_tabulated_form_and_the_workspace_holds_them(reserve):
    L = _lib.lib()
    for (G, rows, Cc, cus), per_elem in ref.REDUCE_CASES.items():
        reserve(cus)
        for elem, want in per_elem.items():
            for p in (BN_PASS_BWD_REDUCE, BN_PASS_EVAL_BWD):
                if p == BN_PASS_EVAL_BWD and elem != FP32:
                    continue
                if want is None:
                    with pytest.raises(RuntimeError, match=ref.REDUCE_REJECTED):
                        ops.bn_plan_query(p, elem, G, rows, Cc)
                    continue
                pl = ops.bn_plan_query(p, elem, G, rows, Cc)
                got = tuple(pl[k] for k in ("cwn", "cw", "column_blocks", "row_lanes", "chunks", "rows_per_chunk", "empty_chunks"))
                assert got == want, ((G, rows, Cc, cus), elem, got)
                # every chunk but the empty ones has rows, and together they cover them exactly once
                assert (pl["chunks"] - pl["empty_chunks"] - 1) * pl["rows_per_chunk"] < rows <= (pl["chunks"] - pl["empty_chunks"]) * pl["rows_per_chunk"]
                have = L.mvg_bn_eval_bwd_workspace_floats(G, rows, Cc) if p == BN_PASS_EVAL_BWD else L.mvg_bn_bwd_workspace_floats(G, rows, Cc)
                assert pl["workspace_floats"] == G * pl["chunks"] * 2 * Cc <= have
            if per_elem[FP32] is not None:                      # the split reduce: fp32 geometry, a third workspace row
                pl = ops.bn_plan_query(BN_PASS_BWD_REDUCE, SP, G, rows, Cc)
                assert tuple(pl[k] for k in ("cwn", "cw", "chunks", "empty_chunks")) == tuple(per_elem[FP32][k] for k in (0, 1, 4, 6))
                assert pl["workspace_floats"] == G * pl["chunks"] * 3 * Cc <= L.mvg_bn_bwd_workspace_floats(G, rows, Cc)
    reserve(0)
    pl = ops.bn_plan_query(BN_PASS_BWD_REDUCE, FP32, 1, 50000, 64)
    assert pl["empty_chunks"] == 10 and 758 * pl["rows_per_chunk"] == 50028 > 50000 > 757 * pl["rows_per_chunk"]


def test_stem_tail_cases_have_the_tabulated_form_and_the_workspace_holds_them(reserve):
    L = _lib.lib()
    for (G, N, H, W, Cc, cus), (train, eval_wgs) in ref.STEM_CASES.items():
        reserve(cus)
        lines = N * ((H - 1) // 2 + 1)
        for elem in (FP32, BF16, SP):
            pl = ops.bn_plan_query(BN_PASS_POOL_BWD_REDUCE, elem, G, 0, Cc, N, H, W)
            assert (pl["chunks"], pl["rows_per_chunk"]) == train and pl["empty_chunks"] == 0, ((G, N, H, W, Cc, cus), pl)
            assert (pl["chunks"] - 1) * pl["rows_per_chunk"] < lines <= pl["chunks"] * pl["rows_per_chunk"]
            assert (pl["cwn"], pl["cw"], pl["row_lanes"]) == (Cc // 4, Cc // 4, 1024 // Cc)       # 4 channels per lane whatever the storage
            assert pl["workspace_floats"] == G * pl["chunks"] * (3 if elem == SP else 2) * Cc <= L.mvg_bn_bwd_workspace_floats(G, N * H * W, Cc)
        pl = ops.bn_plan_query(BN_PASS_POOL_EVAL_BWD, FP32, G, 0, Cc, N, H, W)
        assert pl["chunks"] == eval_wgs and pl["rows_per_chunk"] == 0
        assert pl["workspace_floats"] == G * eval_wgs * 2 * Cc <= L.mvg_bn_eval_bwd_workspace_floats(G, N * H * W, Cc)


def test_finalize_cases_have_the_tabulated_form():
    plenty = 1 << 24
    for (G, P, Cc, scratch), want in ref.FINALIZE_CASES.items():
        pl = ops.bn_plan_query(BN_PASS_FINALIZE, FP32, G, P * 64, Cc, partials=P, scratch_floats=plenty if scratch else 0)
        assert tuple(pl[k] for k in ("form", "lanes_per_group", "slices", "partials_per_slice")) == want, ((G, P, Cc, scratch), pl)
        if pl["slices"]:
            assert (pl["slices"] - 1) * pl["partials_per_slice"] < P <= pl["slices"] * pl["partials_per_slice"] and pl["slices"] <= 64
        # what the query asks for is exactly enough for the fastest form ...
        need = pl["scratch_floats"]
        assert need == (0 if G == 1 and P < 1024 else G * 2 * Cc * 2 + (G * -(-P // -(-P // 64)) * 3 * Cc * 2 if P >= 1024 else 0))
        full = ops.bn_plan_query(BN_PASS_FINALIZE, FP32, G, P * 64, Cc, partials=P, scratch_floats=need)
        assert full == ops.bn_plan_query(BN_PASS_FINALIZE, FP32, G, P * 64, Cc, partials=P, scratch_floats=plenty)
        # ... and one float less is not: unsliced; and, beyond four groups, no per-group form without the records' room
        if P >= 1024:
            less = ops.bn_plan_query(BN_PASS_FINALIZE, FP32, G, P * 64, Cc, partials=P, scratch_floats=need - 1)
            assert less["slices"] == 0 and less["form"] == (ref.PER_GROUP if G > 1 else ref.WALK_GROUPS)
        if G > 4:
            less = ops.bn_plan_query(BN_PASS_FINALIZE, FP32, G, P * 64, Cc, partials=P, scratch_floats=G * 2 * Cc * 2 - 1)
            assert less["form"] == ref.WALK_GROUPS


def test_query_rejects_what_the_launches_reject():
    L = _lib.lib()
    q = ops.bn_plan_query
    for p in (BN_PASS_BWD_REDUCE, BN_PASS_EVAL_BWD, BN_PASS_POOL_BWD_REDUCE):
        with pytest.raises(RuntimeError, match=r"c/4 must divide 256 or be larger than 256 \(c=96\)"):
            q(p, FP32, 1, 100, 96, 1, 10, 10)
    with pytest.raises(RuntimeError, match=r"bn_bwd_reduce: c/8 must divide 256 or be larger than 256 \(c=1536\)"):
        q(BN_PASS_BWD_REDUCE, BF16, 1, 777, 1536)
    assert q(BN_PASS_BWD_REDUCE, FP32, 1, 777, 1536)["column_blocks"] == 2       # accepted: what the old message denied
    with pytest.raises(RuntimeError, match=r"bn_relu_maxpool_eval_bwd: bad sizes \(c/4 must divide 256, c=96\)"):
        q(BN_PASS_POOL_EVAL_BWD, FP32, 1, 0, 96, 1, 10, 10)
    with pytest.raises(RuntimeError, match=r"bn_apply: c % 4 != 0"):
        q(BN_PASS_APPLY, FP32, 1, 10, 6)
    with pytest.raises(RuntimeError, match=r"bn_bwd_apply: c must be a multiple of 8"):
        q(BN_PASS_BWD_APPLY, BF16, 1, 10, 12)
    with pytest.raises(RuntimeError, match=r"bn_apply_split: c % 8 != 0"):
        q(BN_PASS_APPLY, SP, 1, 10, 12)
    with pytest.raises(RuntimeError, match=r"bn_bwd_apply_split: c % 8 != 0"):
        q(BN_PASS_BWD_APPLY, SP, 1, 10, 12)
    with pytest.raises(RuntimeError, match="fp32 only"):
        q(BN_PASS_EVAL_BWD, BF16, 1, 10, 64)
    with pytest.raises(RuntimeError, match="bn_finalize: bad sizes"):
        q(BN_PASS_FINALIZE, FP32, 2, 100, 64, partials=0)
    with pytest.raises(RuntimeError, match="unknown pass"):
        q(9, FP32, 1, 10, 64)
    with pytest.raises(RuntimeError, match="unknown element kind"):
        q(BN_PASS_APPLY, 3, 1, 10, 64)
    with pytest.raises(RuntimeError, match="bad sizes"):
        q(BN_PASS_APPLY, FP32, 0, 10, 64)
    assert L.mvg_bn_plan_query(BN_PASS_APPLY, FP32, 1, 10, 64, 0, 0, 0, 0, 0, None) == 0           # out may be NULL
    assert L.mvg_bn_plan_query(BN_PASS_APPLY, FP32, 1, 10, 6, 0, 0, 0, 0, 0, None) == -1
    # c = 96 streams (apply, bwd-apply) but does not reduce
    assert q(BN_PASS_APPLY, FP32, 1, 48000, 96)["step"] == 16


def test_chunk_count_follows_the_cu_budget(reserve):
    """The CU budget sets the chunk count only above the 64-row floor: the case pair the GPU tests run under both budgets."""
    reserve(0)
    a = ops.bn_plan_query(BN_PASS_BWD_REDUCE, FP32, 1, 5000, 64)
    reserve(16)
    b = ops.bn_plan_query(BN_PASS_BWD_REDUCE, FP32, 1, 5000, 64)
    assert (a["chunks"], b["chunks"]) == (79, 64) and a["rows_per_chunk"] < b["rows_per_chunk"]
    assert ops.bn_plan_query(BN_PASS_APPLY, FP32, 1, 5000, 64) == (reserve(0), ops.bn_plan_query(BN_PASS_APPLY, FP32, 1, 5000, 64))[1]
