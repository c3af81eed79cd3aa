"""The one-pass BatchNorm backward on the running statistics in bf16 storage (csrc/bn.hip: mvg_bn_eval_bwd_bf16 and its stem
tail mvg_bn_relu_maxpool_eval_bwd_bf16), at kernel level - the passes a frozen-BatchNorm training step of the bf16 path runs.

Shapes: every REDUCE_CASES entry of tests/bn_forms_ref.py with a bf16 column (empty trailing chunks; one chunk with exactly one
unrolled trip; unrolled trips plus a tail; 256 column groups with one row lane; the 64-row floor under two CU budgets) and all
six STEM_CASES (odd h / w, c = 8).  The eval-mode plan query stays "fp32 only" for bf16 (tests/test_bn_forms_cpu.py pins that), so
every reduce case FIRST asserts that the BWD_REDUCE / bf16 query - the geometry the bf16 eval pass launches with - still returns
the table's tuple: a moved plan fails loudly instead of testing another form.  The stem tail moves 4 channels per lane in both
storage types: its shapes are guarded through the fp32 POOL_EVAL_BWD query.

Bars, all the project's:
  inputs are rounded to bf16 first; the reference is bn_forms_ref.eval_bwd_ref / stem_tail_ref(train=False) in float64 on those
  rounded values, the ReLU pattern of the affine source taken from the kernels' own forward;
  dz_out         bit-equal to the masked g (a bf16 value or zero: nothing to round);
  dy             bit-equal to the fp32 kernel's dy on the same values, rounded once to bf16 (the element arithmetic IS the fp32
                 kernels': k = gamma / sqrt(running_var + eps), dy = k dz) - and within OUT_RTOL (tests/test_bf16_gpu.py) of float64;
  dgamma, dbeta  held() at SUMS_RTOL, the bar and helper tests/test_bn_forms_gpu.py uses for the bf16 train-mode reduce sums;
  exact counts   gamma = 2, running_var = 1, eps = 0, integer data: dbeta and dgamma are exact integers below 2^24 - a row dropped
                 or counted twice cannot hide behind a tolerance - and dy = 2 g.
Outputs and every workspace start as NaN (poisoned_workspaces): a slot read without having been written shows.
Every comparison prints `BN-FORMS ...` before it asserts, as tests/test_bn_forms_gpu.py does.  Measured on an MI355X (relative
L2 against float64; profiles/r19_frozen_bn_errors.txt): dy 1.6e-03 .. 1.7e-03 (bf16 output rounding), dgamma 7.4e-08 .. 1.6e-07,
dbeta <= 3.2e-08; stem tail dy 1.4e-03 .. 1.7e-03, its sums <= 1.1e-07; 295 comparisons are bit-equalities."""
import pytest
import torch

import bn_forms_ref as ref
from bn_forms_ref import BF16, EPS, FP32, REDUCE_CASES, STEM_CASES
from test_bf16_gpu import OUT_RTOL
from test_bn_forms_gpu import SUMS_RTOL, _reduce_inputs, _winner_values, bf, cus_left, held, nans, poisoned_workspaces, same, store, values
from test_kernels_gpu import dev

pytestmark = pytest.mark.gpu

BF16_REDUCE = [case for case, per in REDUCE_CASES.items() if per[BF16] is not None]
_IDS = ["g%d_r%d_c%d_cus%d" % c for c in BF16_REDUCE]


def _guard(case):
    """Inside cus_left: the bf16 eval pass launches with reduce_geometry(W = 2), what the BWD_REDUCE / bf16 query reports."""
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import BN_PASS_BWD_REDUCE
    G, rows, Cc, cus = case
    pl = ops.bn_plan_query(BN_PASS_BWD_REDUCE, BF16, G, rows, Cc)
    got = tuple(pl[k] for k in ("cwn", "cw", "column_blocks", "row_lanes", "chunks", "rows_per_chunk", "empty_chunks"))
    assert got == REDUCE_CASES[case][BF16], f"reduce {case}: the plan moved this case to {got}"


def _guard_stem(case):
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import BN_PASS_POOL_EVAL_BWD
    G, N, H, W, Cc, cus = case
    pl = ops.bn_plan_query(BN_PASS_POOL_EVAL_BWD, FP32, G, 0, Cc, N, H, W)
    assert pl["chunks"] == STEM_CASES[case][1], f"stem {case}: the plan moved this case to {pl}"


def test_the_cases_are_the_ones_the_table_has():
    assert set(BF16_REDUCE) == {(1, 50000, 64, 0), (2, 64, 64, 0), (1, 37, 256, 0), (3, 1000, 2048, 0), (1, 5000, 64, 0), (1, 5000, 64, 16)}
    assert len(STEM_CASES) == 6


@pytest.mark.parametrize("case", BF16_REDUCE, ids=_IDS)
def test_eval_bwd_bf16_every_mask_source_and_storage_form(case):
    from rot_mvgaze_amd import ops
    G, rows, Cc, cus = case
    u, yd, sc, sh, act_res, bits, masks = _reduce_inputs(BF16, G, rows, Cc)      # (u holds the bf16-rounded values as fp32)
    assert yd.dtype == torch.bfloat16 and bits.numel() == G * rows * Cc // 8
    d = lambda t: t.to(dev())
    god, gd = store(u["go"], BF16), d(u["gamma"])
    rm_h, rv_h = ref.randn((Cc,), 21) * 0.5 + 0.5, ref.randn((Cc,), 22).abs() + 0.5
    rmd, rvd = d(rm_h), d(rv_h)
    # the same values in fp32 storage for the fp32 kernel; the mask bytes of both layouts from the one ReLU pattern
    go32, y32, act32 = d(u["go"]), d(u["y"]), act_res.float()
    on = masks["bits"]
    bits8, bits4 = d(ref.mask_bytes(on, 8)), d(ref.mask_bytes(on, 4))
    same(bits.cpu(), bits8.cpu(), f"bf16 {case} bn_apply_bits bytes == mask_bytes(on, 8)")
    tag = "bf16 g%d_r%d_c%d_cus%d" % case
    with cus_left(cus), poisoned_workspaces():
        _guard(case)
        for src, mask in masks.items():
            e = ref.eval_bwd_ref(u["go"], u["y"], u["gamma"], rm_h, rv_h, EPS, mask)
            kw = {"bits": dict(relu_bits=bits8), "act": dict(act=act_res), "affine": dict(relu_affine=(sc, sh)), "none": {}}[src]
            kw32 = {"bits": dict(relu_bits=bits4), "act": dict(act=act32), "affine": dict(relu_affine=(sc, sh)), "none": {}}[src]
            t = f"{tag} eval-bwd {src}"
            # with dz_out, fresh sums
            dy, dz = nans(G, rows, Cc, dtype=torch.bfloat16), nans(G, rows, Cc, dtype=torch.bfloat16)
            dg, db = nans(Cc), nans(Cc)
            ops.bn_eval_bwd(god, yd, gd, rmd, rvd, EPS, G, rows, Cc, dy, dg, db, False, dz_out=dz, **kw)
            same(dz.cpu(), bf(e["dz"].float()), f"{t} dz_out == masked g")
            dy32, dz32, dg32, db32 = nans(G, rows, Cc), nans(G, rows, Cc), nans(Cc), nans(Cc)
            ops.bn_eval_bwd(go32, y32, gd, rmd, rvd, EPS, G, rows, Cc, dy32, dg32, db32, False, dz_out=dz32, **kw32)
            same(dy, bf(dy32), f"{t} dy == the fp32 kernel's dy rounded once")
            same(dz.float(), dz32, f"{t} dz_out == the fp32 kernel's")
            held(dy.float().cpu(), e["dy"], OUT_RTOL, f"{t} dy")
            held(dg.cpu(), e["dgamma"], SUMS_RTOL, f"{t} dgamma")
            held(db.cpu(), e["dbeta"], SUMS_RTOL, f"{t} dbeta")
            # without dz_out; sums accumulated onto what the buffers hold
            dy2 = nans(G, rows, Cc, dtype=torch.bfloat16)
            pre_g, pre_b = d(ref.randn((Cc,), 41)), d(ref.randn((Cc,), 42))
            dg2, db2 = pre_g.clone(), pre_b.clone()
            ops.bn_eval_bwd(god, yd, gd, rmd, rvd, EPS, G, rows, Cc, dy2, dg2, db2, True, **kw)
            same(dy2, dy, f"{t} dy without dz_out")
            same(dg2, pre_g + dg, f"{t} dgamma accumulated")
            same(db2, pre_b + db, f"{t} dbeta accumulated")
            # dy in place over g, no sums wanted (no finalize launch)
            g3 = god.clone()
            ops.bn_eval_bwd(g3, yd, gd, rmd, rvd, EPS, G, rows, Cc, g3, None, None, False, **kw)
            same(g3, dy, f"{t} dy in place, NULL dgamma / dbeta")
            # dz_out aliasing g, one of the two sums
            g4, dy4, db4 = god.clone(), nans(G, rows, Cc, dtype=torch.bfloat16), nans(Cc)
            ops.bn_eval_bwd(g4, yd, gd, rmd, rvd, EPS, G, rows, Cc, dy4, None, db4, False, dz_out=g4, **kw)
            same(dy4, dy, f"{t} dy with dz in place")
            same(g4, dz, f"{t} dz in place")
            same(db4, db, f"{t} dbeta alone")


@pytest.mark.parametrize("case", BF16_REDUCE, ids=_IDS)
def test_eval_bwd_bf16_counts_every_row_exactly_once(case):
    """g = 1, no mask, integer y and running_mean, running_var = 1 with eps = 0 (invstd_r exactly 1), gamma = 2: dbeta EQUALS
    groups x rows, dgamma the integer sum of (y - running_mean), dy = 2 g and dz_out = g - every value exact in bf16 / fp32."""
    from rot_mvgaze_amd import ops
    G, rows, Cc, cus = case
    gen = torch.Generator().manual_seed(rows + Cc)
    y = torch.randint(-8, 9, (G, rows, Cc), generator=gen).float()
    rm = torch.randint(-3, 4, (Cc,), generator=gen).float()
    g = torch.ones(G, rows, Cc)
    dg_want = (y.double() - rm.double()).sum((0, 1))
    assert float(dg_want.abs().max()) < 2 ** 24 and G * rows * 11 < 2 ** 24
    d = lambda t: t.to(dev())
    yd, gd_ = store(y, BF16), store(g, BF16)
    assert torch.equal(yd.float().cpu(), y)
    tag = "exact bf16 g%d_r%d_c%d_cus%d" % case
    with cus_left(cus), poisoned_workspaces():
        _guard(case)
        dy, dz = nans(G, rows, Cc, dtype=torch.bfloat16), nans(G, rows, Cc, dtype=torch.bfloat16)
        dg, db = nans(Cc), nans(Cc)
        ops.bn_eval_bwd(gd_, yd, d(torch.full((Cc,), 2.0)), d(rm), d(torch.ones(Cc)), 0.0, G, rows, Cc, dy, dg, db, False, dz_out=dz)
        same(db.cpu(), torch.full((Cc,), float(G * rows)), f"{tag} eval-bwd dbeta == groups x rows")
        same(dg.cpu(), dg_want.float(), f"{tag} eval-bwd dgamma")
        same(dy.float().cpu(), 2 * g, f"{tag} eval-bwd dy == gamma g")
        same(dz, gd_, f"{tag} eval-bwd dz_out == g")


def test_eval_bwd_bf16_refuses_what_the_reduce_refuses():
    from rot_mvgaze_amd import ops
    g0 = nans(1, 8, 1536, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match=r"c/8 must divide 256 or be larger than 256 \(c=1536\)"):
        ops.bn_eval_bwd(g0, g0, nans(1536), nans(1536), nans(1536), EPS, 1, 8, 1536, g0.clone(), nans(1536), nans(1536), False)
    g1 = nans(1, 8, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="ONE way"):
        ops.bn_eval_bwd(g1, g1, nans(64), nans(64), nans(64), EPS, 1, 8, 64, g1.clone(), None, None, False, act=g1,
                        relu_affine=(nans(1, 64), nans(1, 64)))
    with pytest.raises(RuntimeError, match="dz_out and dy must be different buffers"):
        dy = g1.clone()
        ops.bn_eval_bwd(g1, g1, nans(64), nans(64), nans(64), EPS, 1, 8, 64, dy, None, None, False, dz_out=dy)


@pytest.mark.parametrize("case", list(STEM_CASES), ids=lambda c: "g%d_n%d_%dx%d_c%d_cus%d" % c)
def test_stem_tail_eval_bwd_bf16(case):
    """mvg_bn_relu_maxpool_eval_bwd_bf16 against autograd through float64 batch_norm(training=False) -> relu -> max_pool2d on
    the bf16-rounded y; negative gamma on some channels.  dy bit-equal to the fp32 kernel's rounded once; a pixel that won no
    window (or whose ReLU is shut) gets exactly zero."""
    from rot_mvgaze_amd import ops
    G, N, H, W, Cc, cus = case
    ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    tag = "stem bf16 g%d_n%d_%dx%d_c%d_cus%d" % case
    y = values(ref.randn((G, N, Cc, H, W), 11 + H) * 1.5 + 0.2, BF16)
    gamma, beta = ref.randn((Cc,), 12) * 0.3 + 1.0, ref.randn((Cc,), 13) * 0.3
    gamma[::7] *= -1
    gp_of = lambda shape: values(ref.randn(shape, 14), BF16)
    nhwc = lambda t: t.permute(0, 1, 3, 4, 2).contiguous()
    d = lambda t: t.to(dev())
    rm_h, rv_h = ref.randn((Cc,), 31) * 0.3 + 0.2, ref.randn((Cc,), 32).abs() + 0.8
    want = ref.stem_tail_ref(y, gamma, beta, gp_of, False, rm_h, rv_h)
    y_nhwc = nhwc(y)
    yd, y32, gd = store(y_nhwc, BF16), d(y_nhwc), d(gamma)
    with cus_left(cus), poisoned_workspaces():
        _guard_stem(case)
        scale, shift = nans(G, Cc), nans(G, Cc)
        ops.bn_eval_affine(G, Cc, gd, d(beta), d(rm_h), d(rv_h), EPS, scale, shift)
        am = torch.full((G, N, ho, wo, Cc), 0xFF, dtype=torch.uint8, device=dev())
        pooled = nans(G, N, ho, wo, Cc, dtype=torch.bfloat16)
        ops.bn_relu_maxpool_fwd(yd, scale, shift, pooled, am, G, N, H, W, Cc, ho, wo)
        held(pooled.float().cpu(), nhwc(want["pooled"]), OUT_RTOL, f"{tag} eval forward")
        gp = nhwc(want["gp"])
        gpd, gp32 = store(gp, BF16), d(gp)
        dy, dg, db = nans(G, N, H, W, Cc, dtype=torch.bfloat16), nans(Cc), nans(Cc)
        ops.bn_relu_maxpool_eval_bwd(gpd, am, yd, scale, shift, gd, d(rm_h), d(rv_h), EPS, G, N, H, W, Cc, ho, wo, dy, dg, db, False)
        dy32, dg32, db32 = nans(G, N, H, W, Cc), nans(Cc), nans(Cc)
        ops.bn_relu_maxpool_eval_bwd(gp32, am, y32, scale, shift, gd, d(rm_h), d(rv_h), EPS, G, N, H, W, Cc, ho, wo, dy32, dg32, db32, False)
        same(dy, bf(dy32), f"{tag} eval dy == the fp32 kernel's dy rounded once")
        held(dy.float().cpu(), nhwc(want["dy"]), OUT_RTOL, f"{tag} eval dy")
        held(dg.cpu(), want["dgamma"], SUMS_RTOL, f"{tag} eval dgamma")
        held(db.cpu(), want["dbeta"], SUMS_RTOL, f"{tag} eval dbeta")
        # untouched pixels: no window's argmax points at them - exactly zero, not a rounding of something small
        _, flat = _winner_values(y_nhwc, am.cpu(), H, W)
        won = torch.zeros(G, N, H * W * Cc).scatter_add_(2, flat.reshape(G, N, -1), torch.ones(G, N, ho * wo * Cc)).reshape(G, N, H, W, Cc)
        lost = won == 0
        assert bool(lost.any())
        same(dy.float().cpu()[lost], torch.zeros(int(lost.sum())), f"{tag} eval dy of pixels that won no window == 0")
        # sums accumulated; and no sums at all
        pre_g, pre_b = d(ref.randn((Cc,), 41)), d(ref.randn((Cc,), 42))
        dy2, dg2, db2 = nans(G, N, H, W, Cc, dtype=torch.bfloat16), pre_g.clone(), pre_b.clone()
        ops.bn_relu_maxpool_eval_bwd(gpd, am, yd, scale, shift, gd, d(rm_h), d(rv_h), EPS, G, N, H, W, Cc, ho, wo, dy2, dg2, db2, True)
        same(dy2, dy, f"{tag} eval dy again")
        same(dg2, pre_g + dg, f"{tag} eval dgamma accumulated")
        same(db2, pre_b + db, f"{tag} eval dbeta accumulated")
        dy3 = nans(G, N, H, W, Cc, dtype=torch.bfloat16)
        ops.bn_relu_maxpool_eval_bwd(gpd, am, yd, scale, shift, gd, d(rm_h), d(rv_h), EPS, G, N, H, W, Cc, ho, wo, dy3, None, None, False)
        same(dy3, dy, f"{tag} eval dy, NULL dgamma / dbeta")


def test_stem_tail_eval_bwd_bf16_refuses_c96():
    from rot_mvgaze_amd import ops
    y = nans(1, 1, 4, 4, 96, dtype=torch.bfloat16)
    gp = nans(1, 1, 2, 2, 96, dtype=torch.bfloat16)
    am = torch.zeros(1, 1, 2, 2, 96, dtype=torch.uint8, device=dev())
    with pytest.raises(RuntimeError, match=r"bn_relu_maxpool_eval_bwd: bad sizes \(c/4 must divide 256, c=96\)"):
        ops.bn_relu_maxpool_eval_bwd(gp, am, y, nans(1, 96), nans(1, 96), nans(96), nans(96), nans(96), EPS, 1, 1, 4, 4, 96, 2, 2,
                                     y.clone(), None, None, False)
