"""The two kernels of a frozen-BatchNorm step on the split kernels (csrc/bn.hip) at kernel level, against float64.

mvg_bn_frozen_finalize     one launch per unit in place of mvg_bn_eval_affine: (scale, shift) with that entry point's bits, mean /
                           invstd := the running values broadcast over the groups, the unit's chained activation bound from the conv
                           epilogue's statistics partials, and the 2^-k of its sp output.
mvg_bn_frozen_bwd_apply_split   dy = sp(gamma invstd dz 2^k), one pass: g already masked / the mask from y / no ReLU.

References: tests/frozen_split_ref.py (tests/test_frozen_split_cpu.py holds it to float64 truth), float64 formulas on the kernels'
own fp32 inputs.  Outputs start as NaN.  Bars - none fitted to the kernels:
  scale, shift     torch.equal to ops.bn_eval_affine's;  mean torch.equal to the running mean;  invstd within 2^-22 relative of
                   the float64 1 / sqrt(rv + eps) (three correctly rounded fp32 operations: add, sqrt, divide)
  bound            >= the float64 maximum of |the normalised tensor| (+ the identity's bound): a bound holds or it does not;
                   <= (the float64 formula x MARGIN + identity) x (1 + 2^-16): MARGIN = 1 + 2^-7 is the kernel's stated factor; the
                   rest covers the fp32 rounding of the partials handed to the kernel (2^-24 of each sum, well-conditioned here:
                   |mean| and the spread are of one size), of the bound's conversion to fp32 and of the chained sum (2^-24 each)
  slot             exactly the power of two frozen_split_ref.sinv_for gives for the kernel's own bound
  frozen apply     the per-element bar tests/test_bn_forms_gpu.py applies to mvg_bn_bwd_apply_split (the final rounding - the sp
                   split - is the same): close() at SUMS_RTOL = 1e-4 and every element within 1e-6 of the maximum, here against
                   float64 directly; the stored pieces below fp16's 65 504.
Every comparison prints a `FROZEN-SPLIT ...` line before it asserts.  Measured on an MI355X (profiles/frozen_split_errors.txt; no bar
was fitted to these): invstd <= 1.4 x 2^-24 of float64; the bound 1.95 .. 2.34 x the true maximum and within 8e-8 of the float64
formula x MARGIN; every slot the rule's power of two; the frozen apply 7.5e-08 .. 1.3e-07 of the maximum per element."""
import math

import numpy as np
import pytest
import torch

import frozen_split_ref as ref
from test_bn_forms_gpu import SUMS_RTOL, nans, sp_nans
from test_kernels_gpu import close, dev

pytestmark = pytest.mark.gpu

EPS = 1e-5
G, ROWS, RPP = 2, 98, 40          # 2 x 7 x 7 rows per group: no multiple of a tile; partials of 40 + 40 + 18 rows


def _unit(c, seed, regime):
    """Conv outputs and a BatchNorm whose running statistics do not describe them (mean shifted by three spreads, variance
    shrunken to 5 %).  regime: where the bound falls - "band" [1, 2^15), "big" beyond it, "small" below 1."""
    rng = np.random.default_rng(seed)
    spread = np.exp(rng.standard_normal(c) * 0.5)
    y = (rng.standard_normal((G, ROWS, c)) * spread + rng.standard_normal(c) * 2).astype(np.float32)
    k = {"band": 1.0, "big": 3.0e4, "small": 1.0e-4}[regime]
    gamma = (rng.standard_normal(c) * 1.5 * k).astype(np.float32)
    beta = (rng.standard_normal(c) * k).astype(np.float32)
    rm = (y.mean((0, 1)) + 3 * spread * rng.choice([-1.0, 1.0], c)).astype(np.float32)
    rv = (y.var((0, 1)) * 0.05).astype(np.float32)
    return y, gamma, beta, rm, rv


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


@pytest.mark.parametrize("regime", ["band", "big", "small"])
@pytest.mark.parametrize("ident", [False, True], ids=["no-identity", "identity"])
@pytest.mark.parametrize("c", [32, 64])
def test_frozen_finalize(c, ident, regime):
    from rot_mvgaze_amd import ops
    y, gamma, beta, rm, rv = _unit(c, 1000 + c, regime)
    stats = ref.partials(y, RPP)
    assert stats.shape == (G, 3, 2, c) and ROWS % RPP != 0
    gd, bd, rmd, rvd = _d(gamma), _d(beta), _d(rm), _d(rv)
    rm0, rv0 = rmd.clone(), rvd.clone()
    ident_bound = 12.5 * {"band": 1.0, "big": 3.0e4, "small": 1.0e-4}[regime] if ident else 0.0
    ident_rec = torch.tensor([0.0, 0.0, ident_bound, 0.0], device=dev())
    for with_slot in (True, False):                         # (False: a downsample unit - a bound, no slot)
        mean, invstd, scale, shift = nans(G, c), nans(G, c), nans(G, c), nans(G, c)
        state = torch.zeros(4, device=dev())
        slot = nans(1) if with_slot else None
        ops.bn_frozen_finalize(_d(stats), G, 3, RPP, ROWS, c, gd, bd, rmd, rvd, EPS, mean, invstd, scale, shift, state, slot,
                               ident_rec[2:3] if ident else None)
        torch.cuda.synchronize()
        tag = f"finalize c{c} {'identity' if ident else 'no-identity'} {regime} {'slot' if with_slot else 'no-slot'}"
        # the constants
        want_scale, want_shift = nans(G, c), nans(G, c)
        ops.bn_eval_affine(G, c, gd, bd, rmd, rvd, EPS, want_scale, want_shift)
        assert torch.equal(scale, want_scale) and torch.equal(shift, want_shift), tag
        assert torch.equal(mean, rmd[None].expand(G, c)), tag
        is64 = ref.invstd_running(rv, EPS)
        e = float(np.abs(invstd.cpu().double().numpy() / is64[None] - 1).max())
        print(f"FROZEN-SPLIT {tag}: invstd {e / 2.0 ** -24:.2f} x 2^-24 of float64 (bar 4)")
        assert e <= 2.0 ** -22, tag
        # the running statistics are read, never written
        assert torch.equal(rmd, rm0) and torch.equal(rvd, rv0), tag
        # the bound
        got = float(state[2])
        true = float(np.abs(ref.normalised(y, gamma, beta, rm, rv, EPS)).max()) + ident_bound
        formula = ref.unit_bound(y, gamma, beta, rm, rv, EPS)
        upper = (formula * ref.MARGIN + ident_bound) * (1 + 2.0 ** -16)
        print(f"FROZEN-SPLIT {tag}: bound {got:.6e}, true maximum {true:.6e} (x {got / true:.4f}), float64 formula x margin "
              f"{formula * ref.MARGIN + ident_bound:.6e} (x {got / (formula * ref.MARGIN + ident_bound):.8f})")
        assert math.isfinite(got) and got >= true, tag
        assert got <= upper, tag
        if with_slot:
            want = ref.sinv_for(got)
            print(f"FROZEN-SPLIT {tag}: slot 2^{math.log2(float(slot)):.0f}, the rule gives 2^{math.log2(want):.0f}")
            assert float(slot) == want, tag
            assert (want == 1.0) == (regime == "band"), tag
            assert got * (1.0 / want) < 2.0 ** 15 and (regime == "band" or got * (1.0 / want) >= 2.0 ** 14), tag
        # the arrival count: every workgroup (c / 8 per group) came by exactly once
        assert int(state[1:2].view(torch.int32)) == (c // 8) * G, tag


def test_frozen_finalize_gives_scale_one_for_a_bound_it_cannot_state():
    """An infinite gamma (and a NaN beta) make the bound infinite: the slot is 1, nothing else is poisoned."""
    from rot_mvgaze_amd import ops
    c = 32
    y, gamma, beta, rm, rv = _unit(c, 5, "band")
    gamma[3], beta[7] = np.inf, np.nan
    mean, invstd, scale, shift = nans(G, c), nans(G, c), nans(G, c), nans(G, c)
    state, slot = torch.zeros(4, device=dev()), nans(1)
    ops.bn_frozen_finalize(_d(ref.partials(y, RPP)), G, 3, RPP, ROWS, c, _d(gamma), _d(beta), _d(rm), _d(rv), EPS, mean, invstd, scale,
                           shift, state, slot)
    assert float(state[2]) == math.inf and float(slot) == 1.0
    assert bool(torch.isfinite(invstd).all()) and bool(torch.isfinite(mean).all())


def test_frozen_finalize_rejects_partials_that_do_not_cover_the_rows():
    from rot_mvgaze_amd import ops
    c = 32
    t = lambda *s: torch.zeros(*s, device=dev())
    with pytest.raises(RuntimeError, match="do not cover"):
        ops.bn_frozen_finalize(t(G, 2, 2, c), G, 2, RPP, ROWS, c, t(c), t(c), t(c), t(c), EPS, t(G, c), t(G, c), t(G, c), t(G, c), t(4))


@pytest.mark.parametrize("keep_dz", [False, True], ids=["dy-only", "keeps-dz"])
@pytest.mark.parametrize("form", ["masked", "affine", "no-relu"])
@pytest.mark.parametrize("c", [32, 64])
def test_frozen_bwd_apply(c, form, keep_dz):
    """form: "masked" g already masked (a residual unit: the reduce pass left dz in g - with keep_dz that pass really runs, on the
    running (mean, invstd), and its sums are dbeta / dgamma), "affine" the mask rebuilt from y, "no-relu" a downsample unit.
    keep_dz: the residual branch reads dz from g afterwards - g must come out of the apply pass bit-unchanged."""
    from rot_mvgaze_amd import ops
    y, gamma, beta, rm, rv = _unit(c, 2000 + c, "band")
    rng = np.random.default_rng(c)
    g = (rng.standard_normal((G, ROWS, c)) * np.exp(rng.standard_normal(c))).astype(np.float32)
    is32 = (1.0 / np.sqrt(rv + np.float32(EPS))).astype(np.float32)
    invstd = np.broadcast_to(is32, (G, c)).copy()
    scale = (gamma / np.sqrt(rv + np.float32(EPS))).astype(np.float32)
    shift = (beta - rm * scale).astype(np.float32)
    on = (y.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64)) > 0     # the sign fma(y, scale, shift) has
    dz = g.astype(np.float64) * on if form != "no-relu" else g.astype(np.float64)
    want = gamma.astype(np.float64) * invstd.astype(np.float64)[:, None, :] * dz
    tag = f"bwd-apply c{c} {form} {'keeps-dz' if keep_dz else 'dy-only'}"
    yd, isd, gd = _d(y), _d(invstd), _d(gamma)
    sc, sh = _d(np.broadcast_to(scale, (G, c)).copy()), _d(np.broadcast_to(shift, (G, c)).copy())
    dy = sp_nans(G, ROWS, c)
    if form == "masked" and keep_dz:
        # the pair as the backbone runs it for a residual unit: bits -> the reduce pass masks g in place and leaves the scale
        bits = _d(np.packbits(on.reshape(G, ROWS, c // 4, 4), axis=-1, bitorder="little").reshape(-1))
        gin = _d(g)
        s12, sinv = nans(3, G, c), nans(1)
        dgam, dbet = nans(c), nans(c)
        ops.bn_bwd_reduce_split(gin, bits, yd, _d(np.broadcast_to(rm, (G, c)).copy()), isd, G, ROWS, c, s12[0], s12[1], dgam, dbet, False,
                                s12[2], None, dz_out=gin, gamma=gd, dy_sinv=sinv)
        xhat = (y.astype(np.float64) - rm.astype(np.float64)) * invstd.astype(np.float64)[:, None, :]
        close(dbet.cpu(), torch.from_numpy(dz.sum((0, 1))), SUMS_RTOL, f"{tag} dbeta")
        close(dgam.cpu(), torch.from_numpy((dz * xhat).sum((0, 1))), SUMS_RTOL, f"{tag} dgamma")
        assert torch.equal(gin.cpu(), torch.from_numpy(dz.astype(np.float32))), f"{tag}: dz in g"
    else:
        gin = _d(dz.astype(np.float32)) if form == "masked" else _d(g)
        bound = float(np.abs(gamma.astype(np.float64) * invstd.astype(np.float64)).max() * np.abs(g).max())
        sinv = torch.tensor([2.0 ** (math.frexp(bound)[1] - 15)], device=dev())     # elem.h: sp_scale_for - the bound just below 2^15
    before = gin.clone()
    ops.bn_frozen_bwd_apply_split(gin, yd, isd, gd, G, ROWS, c, dy, sinv, (sc, sh) if form == "affine" else None)
    torch.cuda.synchronize()
    assert dy.sinv is sinv
    got = ops.merge_sp(dy).cpu().double()
    assert bool(torch.isfinite(got).all()), f"{tag}: an element no lane wrote"
    wt = torch.from_numpy(want)
    e = float((got - wt).abs().max() / wt.abs().max())
    l2 = float((got - wt).norm() / wt.norm())
    print(f"FROZEN-SPLIT {tag}: max error {e:.3e} of the maximum (bar 1e-6), rel-L2 {l2:.3e}, dy scale 2^{-math.log2(float(sinv)):.0f}")
    close(got, wt, SUMS_RTOL, tag)
    assert e <= 1e-6, tag
    assert float(dy.float().abs().max()) < 65504.0, tag
    # the true dy fits the scale the reduce pass chose (its bound only adds non-negative terms to |gamma invstd| max |dz|)
    assert float(wt.abs().max()) / float(sinv) < 65504.0, tag
    if keep_dz:
        assert torch.equal(gin, before), f"{tag}: the pass wrote to g"


def test_frozen_bwd_apply_rejects_half_a_mask_and_odd_channel_counts():
    from rot_mvgaze_amd import ops
    t = lambda *s: torch.zeros(*s, device=dev())
    one = torch.ones(1, device=dev())
    with pytest.raises(RuntimeError, match="c % 8"):
        ops.bn_frozen_bwd_apply_split(t(1, 8, 12), t(1, 8, 12), t(1, 12), t(12), 1, 8, 12, ops.sp_empty(1, 8, 16, device=dev()), one)
