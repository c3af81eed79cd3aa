"""The fusion block's Linears on the split kernels - mvg_linear_fprop_split / _dgrad_split (igemm_split16_kernel<BN, DGRAD, LIN = true,
2, STAGES>: eight instantiations with their own epilogue branches) and mvg_linear_wgrad_split (wgrad_split_kernel<.., incremental =
false>, both operands scaled) - and the operand builders around them (mvg_split_colsum, mvg_absmax_multi, mvg_fuse_build_split,
mvg_fuse_unbuild), at kernel level on small shapes.  tests/fusion_split_forms_ref.py holds the case tables, the inputs, the float64
references and the derived bars; tests/test_fusion_split_forms_cpu.py checks those on their own.

Conventions of test_prep_forms_gpu.py: every output starts as NaN inside a larger allocation whose sentinel margins must be
bit-unchanged afterwards (`Guarded`); every abs-max / 2^-k slot starts at 0, as the callers' contract asks; every Linear case FIRST
asserts, through the host-only query mvg_linear_plan_query_split (answered by the code the launches plan with), which instantiation
it is about to run under each of three settings of ops.set_reserved_cus (every CU, 16 CUs, 8 CUs: the plan moves, not the shape), and
the last test holds the union of the forms seen to fusion_split_forms_ref.FORMS; every comparison prints its figure as
`FUSION-SPLIT-FORMS <kernel> <case> <form>: ...` before it asserts.

Conditions - taken from the project or derived, none fitted to the kernels:
  Linear forward: (a) the fp32 result within SPLIT_VS_F64 (relative L2) and per element close(.., 2e-5) of float64 x W^T + b on the
      values the sp operands hold; its abs-max slot holds the bits of max |y| of the device result, and a slot pre-set above stays.
      (b), (c) an sp result with ReLU: *out_sinv = 1 / sp_scale_for(fp32(fin * 2^30 * x_sinv * w_sinv) [+ bias_absmax]) exactly, and
      the stored pieces are the host pieces of relu(y_a) / out_sinv (the sp condition of test_prep_forms_gpu.py) - the same
      instantiation and accumulators as (a), a runtime branch in the epilogue.  (d) the fp32 result with ReLU equals relu(y_a).
  Linear backward-data: plain as (a); with the sp ReLU mask of a forward equal to where(merge_sp(h) > 0, dx, 0); with an addend equal
      to dx + addend in fp32; with both the mask first; the abs-max slot of a masked launch holds the maximum of the masked result.
  Across settings: results of one shape under the same column tile are torch.equal whichever K loop ran (both multiply the same
      fragments in ascending K-step order and share one epilogue: test_split_forms_gpu.py).
  Linear weight gradient: every tile, x at 1e3 and dy at 1e-3 (both 2^-k != 1), fresh and accumulating, under the slab counts of every CU
      and of 8 CUs: as (a) against float64 g^T x (+ the starting dw) on the values the operands hold.
  split_colsum: *out_sinv = 1 / sp_scale_for(max |g|) exactly; the pieces under the sp condition; db per element within
      (ceil(rows / 64) + 64) * 2^-24 * (sum_r |g| + |db0|) of the float64 column sum; two runs and a run without db give the same bits.
  absmax_multi: every slot holds the bits of max |x|; a zero count and an all-zero tensor leave their slot alone; a higher slot stays.
  fuse_build_split: both 2^-k exact; copied columns under the sp condition; rotated columns per element within
      3 * 2^-24 * sum_j |r_aj f_j| + 2^-23 |want| + 2^-25 * 2^-k of float64.
  fuse_unbuild: dF and da per element within terms * 2^-24 * sum |terms| of float64; the slot holds the bits of max |dF|.

Measured on an MI355X (profiles/fusion_split_forms_errors.txt), smallest .. largest over the cases; no bar above was refitted to them:
  Linear forward y (39 comparisons), relative L2      6.4e-08 .. 4.1e-07 (bar 2e-6); largest element error 1.0e-07 .. 9.0e-07 of max |ref| (bar 2e-5)
  Linear forward sp results (78)                      pieces differing from the host pieces of relu(y_a) / out_sinv 0 .. 0; out_sinv bits differing 0 .. 0;
                                                      fp32 + ReLU elements differing from relu(y_a) 0 .. 0; abs-max slots off their maximum 0 .. 0 (of 39)
  Linear backward-data dx (39), relative L2           6.2e-08 .. 4.3e-07 (bar 2e-6); largest element error 9.2e-08 .. 1.1e-06 (bar 2e-5)
  ... mask / addend / mask + addend (117)             elements differing from the fp32 expression on the plain dx 0 .. 0; slots off 0 .. 0 (of 78)
  across settings (40 pairs)                          every pair under one column tile equal, whichever K loop ran
  Linear weight gradient (40), relative L2            4.6e-08 .. 2.6e-07 (bar 2e-6); largest element error 6.1e-08 .. 5.2e-07 (bar 2e-5); 1, 2 and 4 slabs
  split_colsum (46 inputs)                            db at 0 .. 0.053 of its bound, accumulating 0 .. 0.051; pieces differing 0 .. 0; 2^-k bits differing 0 .. 0
  absmax_multi (8 slots, two launches)                slots differing from the bits of max |x| 0 .. 0
  fuse_build_split (24 launches)                      rotated columns at 0.58 .. 0.77 of their bound; copied columns differing 0 .. 0 (56 comparisons); 2^-k exact
  fuse_unbuild (27 cases)                             dF at 0 .. 0.53 and da at 0.17 .. 0.55 of their bounds; slots off max |dF| 0 .. 0
  sp comparisons, 180 in all: subnormal-piece elements that differed 0 .. 0 - the exception was never used

What the cases taught.  No kernel was found wrong.  Six deliberate one-line changes of the kernels (the abs-max of a Linear epilogue without
its last wave, `>= 0` in the sp ReLU mask, split_colsum without its last row lane, fuse_build_split without the second piece of the image
chunks past 256, fuse_unbuild's abs-max without the third axis, absmax_multi without its second grid pass) each failed the tests named
for them here (40 of the 104), on a library built for that one run.  A tensor
with no elements has a null data pointer, which mvg_absmax_multi refuses: the zero count goes in through the library with a live
pointer.  And `randn * 0` holds -0.0, which split_colsum stores as -0.0, as the host pieces do: the all-zero gradient is torch.zeros.
"""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest
import torch

import rot_mvgaze_amd  # noqa: F401
import fusion_split_forms_ref as R
from test_kernels_gpu import close, dev  # noqa: F401  (close: the per-element bar inside held_f32)
from test_prep_forms_gpu import Guarded, L, bits32, held_f32, held_sp, p, st, u16
from test_split_forms_gpu import reserved_cus
from test_split_gpu import SPLIT_VS_F64, rel_l2  # noqa: F401  (the bars inside held_f32)

pytestmark = pytest.mark.gpu

TAG = "FUSION-SPLIT-FORMS"
_seen = set()


def relabelled(fn, *args, **kw):
    """fn (held_f32 / held_sp of test_prep_forms_gpu.py: they print their figures, then assert) with its lines under this file's tag."""
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            return fn(*args, **kw)
    finally:
        print(buf.getvalue().replace("PREP-FORMS", TAG), end="")


def settings():
    cus = L().mvg_device_cus()
    assert cus == R.DEVICE_CUS, f"the case tables are written for a {R.DEVICE_CUS}-CU device (this one has {cus})"
    return R.settings(cus)


def slot(value=0.0):
    return Guarded((1,), init=float(value))


def sp_out(rows, cols, sinv_slot):
    out = Guarded((rows, cols // 8, 2, 8), torch.float16)
    out.t.sinv = sinv_slot.t
    return out


def split_scaled(t):
    """t on the device and its sp copy times the 2^k its abs-max allows (mvg_split_f32: tests/test_prep_forms_gpu.py)."""
    from rot_mvgaze_amd import ops
    return ops.split_f32(t.to(dev()).contiguous(), R.scale_of(t))


def weights_sp(w):
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import ConvDesc
    fout, fin = w.shape
    return ops.split_weights(ConvDesc.linear(1, fin, fout), w.to(dev()).contiguous(), True)


def held64(t_sp):
    """float64, on the host, of what an sp tensor holds (mvg_merge_sp: the pieces' sum times the tensor's 2^-k)."""
    from rot_mvgaze_amd import ops
    return ops.merge_sp(t_sp).double().cpu()


def same_bits(a, b):
    return bool((bits32(a) == bits32(b)).all())


def slot_holds_max(sl, result, what):
    """The abs-max slot holds the bits of max |result| of the device result."""
    got, want = int(bits32(sl.intact(what + " slot"))[0]), int(bits32(result.abs().max().reshape(1))[0])
    print(f"{TAG} {what}: abs-max slot {got:#010x} (max |result| {want:#010x})")
    assert got == want, f"{what}: the slot does not hold max |result|"


def bound_ratio(got, ref, bound):
    """The largest |got - ref| / bound (float64 tensors); an element whose bound is 0 must be exact."""
    err = (got.double().cpu() - ref).abs()
    assert bool(torch.isfinite(err).all()), "non-finite values (an element the launch did not write)"
    exact = bound == 0
    if bool((err[exact] != 0).any()):
        return float("inf")
    return float((err[~exact] / bound[~exact]).max()) if bool((~exact).any()) else 0.0


def cid(shape):
    return "x".join(map(str, shape))


# ---------------------------------------------------------------- Linear forward
@pytest.mark.parametrize("shape,forms,why", R.LINEAR_CASES, ids=[cid(c[0]) for c in R.LINEAR_CASES])
def test_fusion_split_forms_linear_forward(shape, forms, why):
    from rot_mvgaze_amd import ops
    rows, fin, fout = shape
    inp = R.linear_inputs(rows, fin, fout)
    xs, (wk, _) = split_scaled(inp.x), weights_sp(inp.w)
    b = inp.b.to(dev())
    bam = b.abs().max().reshape(1)
    x_sinv, w_sinv = float(xs.sinv), float(wk.sinv)
    assert x_sinv != 1.0 and w_sinv != 1.0
    ref = held64(xs) @ held64(wk).t() + inp.b.double()
    got = {}
    for (name, res), (bn, stages) in zip(settings(), forms):
        what = f"linear_fprop {cid(shape)} <{bn},{stages}-stage> ({name})"
        with reserved_cus(res):
            plan = ops.linear_plan_query_split(rows, fin, fout)
            assert plan == (128, bn, stages), f"{what}: this shape moved to {plan}"
            _seen.add(("linear", bn, stages, False))
            y, am = Guarded((rows, fout)), slot()
            ops.linear_fprop_split(xs, wk, b, False, y.t, rows, fin, fout, out_absmax=am.t)
            top = float(y.t.abs().max())
            y2, am2 = Guarded((rows, fout)), slot(2.0 * top)
            ops.linear_fprop_split(xs, wk, b, False, y2.t, rows, fin, fout, out_absmax=am2.t)
            hb_s, hc_s = slot(), slot()
            hb, hc = sp_out(rows, fout, hb_s), sp_out(rows, fout, hc_s)
            ops.linear_fprop_split(xs, wk, b, True, hb.t, rows, fin, fout, bias_absmax=bam)
            ops.linear_fprop_split(xs, wk, b, True, hc.t, rows, fin, fout)
            yr = Guarded((rows, fout))
            ops.linear_fprop_split(xs, wk, b, True, yr.t, rows, fin, fout)
        # (a)
        relabelled(held_f32, y, ref, what + " y", split=True)
        slot_holds_max(am, y.t, what + " y")
        kept = same_bits(am2.intact("slot"), torch.tensor([2.0 * top]))
        print(f"{TAG} {what} y: a slot pre-set to twice the maximum is unchanged {kept}, the result is the same {torch.equal(y2.intact('y'), y.t)}")
        assert kept and torch.equal(y2.t, y.t)
        # (b), (c)
        relu_ya = torch.relu(y.t).cpu().numpy()
        for tag, h, hs, bias_am in (("sp+relu+bias_absmax", hb, hb_s, float(bam)), ("sp+relu", hc, hc_s, 0.0)):
            bound, want_sinv = R.lin_out_sinv(fin, x_sinv, w_sinv, bias_am)
            got_sinv = hs.intact("out_sinv").cpu().numpy()[0]
            print(f"{TAG} {what} {tag}: out_sinv {got_sinv!r} (host {want_sinv!r} from the bound {bound!r})")
            assert got_sinv.view(np.uint32) == want_sinv.view(np.uint32), f"{what} {tag}: out_sinv is not 2^-k of the bound"
            stored = relu_ya * (np.float32(1.0) / want_sinv)
            assert float(stored.max()) < 2.0 ** 15
            relabelled(held_sp, h, stored, f"{what} {tag}")
        # (d)
        same = torch.equal(yr.intact(what + " relu"), torch.relu(y.t))
        print(f"{TAG} {what} fp32+relu: equal to relu(y) {same}")
        assert same
        got.setdefault(bn, []).append((name, stages, (y.t, hb.t, hc.t, yr.t, am.t, hb_s.t, hc_s.t)))
    across_settings(got, f"linear_fprop {cid(shape)}")


def across_settings(got, what):
    for bn, runs in got.items():
        for name, stages, outs in runs[1:]:
            same = all(torch.equal(a.view(torch.int16) if a.dtype == torch.float16 else a, b.view(torch.int16) if b.dtype == torch.float16 else b)
                       for a, b in zip(outs, runs[0][2]))
            print(f"{TAG} {what} <{bn},*>: {name} ({stages}-stage) equals {runs[0][0]} ({runs[0][1]}-stage) {same}")
            assert same, f"{what}: {bn}-column results differ between {name} and {runs[0][0]}"


# ---------------------------------------------------------------- Linear backward-data
@pytest.mark.parametrize("shape,forms,why", R.LINEAR_CASES, ids=[cid(c[0]) for c in R.LINEAR_CASES])
def test_fusion_split_forms_linear_backward_data(shape, forms, why):
    """The mirrored Linear: [rows, fout'] <- [rows, fin'] with fin' = the table row's fout in the column role."""
    from rot_mvgaze_amd import ops
    rows, fout, fin = shape
    inp = R.linear_inputs(rows, fin, fout)
    gs, (_, wt) = split_scaled(inp.g), weights_sp(inp.w)
    ref = held64(gs) @ held64(wt).t()                         # wt: [fin, fout] in sp, what the launch reads
    addend = inp.addend.to(dev())
    # the mask: the sp ReLU output [rows, fin] of a forward, with its bound-derived scale
    x0s, (w0k, _), b0 = split_scaled(inp.x0), weights_sp(inp.w0), inp.b0.to(dev())
    h = ops.sp_empty(rows, fin, device=dev())
    h.sinv = torch.zeros(1, device=dev())
    ops.linear_fprop_split(x0s, w0k, b0, True, h, rows, 32, fin, bias_absmax=b0.abs().max().reshape(1))
    on = ops.merge_sp(h) > 0
    share = float(on.float().mean())
    assert 0.2 < share < 0.8, "a mask that passes or blocks almost everything tests little"
    got = {}
    for (name, res), (bn, stages) in zip(settings(), forms):
        what = f"linear_dgrad {cid((rows, fin, fout))} <{bn},{stages}-stage> ({name})"
        with reserved_cus(res):
            plan = ops.linear_plan_query_split(rows, fin, fout, dgrad=True)
            assert plan == (128, bn, stages), f"{what}: this shape moved to {plan}"
            _seen.add(("linear", bn, stages, True))
            dx, dxm, dxa, dxma = (Guarded((rows, fin)) for _ in range(4))
            am, amm = slot(), slot()
            ops.linear_dgrad_split(gs, wt, dx.t, rows, fin, fout, out_absmax=am.t)
            top = float(dx.t.abs().max())
            dx2, am2 = Guarded((rows, fin)), slot(2.0 * top)
            ops.linear_dgrad_split(gs, wt, dx2.t, rows, fin, fout, out_absmax=am2.t)
            ops.linear_dgrad_split(gs, wt, dxm.t, rows, fin, fout, relu_mask_sp=h, out_absmax=amm.t)
            ops.linear_dgrad_split(gs, wt, dxa.t, rows, fin, fout, addend=addend)
            ops.linear_dgrad_split(gs, wt, dxma.t, rows, fin, fout, addend=addend, relu_mask_sp=h)
        relabelled(held_f32, dx, ref, what + " dx", split=True)
        slot_holds_max(am, dx.t, what + " dx")
        kept = same_bits(am2.intact("slot"), torch.tensor([2.0 * top]))
        print(f"{TAG} {what} dx: a slot pre-set to twice the maximum is unchanged {kept}, the result is the same {torch.equal(dx2.intact('dx'), dx.t)}")
        assert kept and torch.equal(dx2.t, dx.t)
        masked = torch.where(on, dx.t, torch.zeros_like(dx.t))
        checks = (("mask", dxm, masked), ("addend", dxa, dx.t + addend), ("mask+addend", dxma, masked + addend))
        for tag, out, want in checks:
            differ = int((out.intact(f"{what} {tag}") != want).sum())
            print(f"{TAG} {what} {tag}: elements differing from the fp32 expression on the plain dx {differ} of {want.numel()} (mask passes {share:.2f})")
            assert differ == 0 and bool(torch.isfinite(out.t).all()), f"{what} {tag}"
        slot_holds_max(amm, dxm.t, what + " mask")
        got.setdefault(bn, []).append((name, stages, (dx.t, dxm.t, dxa.t, dxma.t, am.t, amm.t)))
    across_settings(got, f"linear_dgrad {cid((rows, fin, fout))}")


# ---------------------------------------------------------------- Linear weight gradient
@pytest.mark.parametrize("shape,tile,slabs_differ", R.WGRAD_CASES, ids=[cid(c[0]) for c in R.WGRAD_CASES])
def test_fusion_split_forms_linear_weight_gradient(shape, tile, slabs_differ):
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import ConvDesc
    rows, fin, fout = shape
    d = ConvDesc.linear(rows, fin, fout)
    assert ops.conv_wgrad_split_tile(d) == tile + (False,), "this shape no longer runs the tile (decoded pixel addressing) it is here for"
    _seen.add(("wgrad",) + tile)
    gn = R.gen(rows, fin, fout, 3)
    x, g = torch.randn(rows, fin, generator=gn) * 1e3, torch.randn(rows, fout, generator=gn) * 1e-3
    dw0 = torch.randn(fout, fin, generator=gn) * rows ** 0.5
    xs, gs = split_scaled(x), split_scaled(g)
    assert float(xs.sinv) != 1.0 and float(gs.sinv) != 1.0
    ref = held64(gs).t() @ held64(xs)
    slabs = []
    all_cus, _, eight = settings()
    for name, res in (all_cus, eight):
        for accumulate in (False, True):
            with reserved_cus(res):
                splits = L().mvg_conv_wgrad_splits_split(C.byref(d))
                assert splits >= 1
                dw = Guarded((fout, fin), init=dw0 if accumulate else None)
                ws = Guarded((splits * fout * fin,)) if splits > 1 else None
                rc = L().mvg_linear_wgrad_split(rows, fin, fout, p(xs), p(xs.sinv), p(gs), p(gs.sinv), p(dw.t), p(ws.t) if ws else None, splits,
                                                int(accumulate), st())
            from rot_mvgaze_amd._lib import check
            check(rc, "linear_wgrad_split")
            if ws:
                ws.intact("slabs")
            what = f"linear_wgrad {cid(shape)} {tile[0]}x{tile[1]} ({name}, {splits} slabs, accumulate={accumulate})"
            relabelled(held_f32, dw, ref + dw0.double() if accumulate else ref, what, split=True)
        slabs.append(splits)
    if slabs_differ:
        assert slabs[0] > slabs[1], f"slab counts {slabs}: the two settings no longer sum this shape differently"


# ---------------------------------------------------------------- split_colsum
def colsum_run(g, rows, cols, am, db0=None, with_db=True):
    from rot_mvgaze_amd import ops
    sinv = slot()
    out = sp_out(rows, cols, sinv)
    db = Guarded((cols,), init=db0 if db0 is not None else None) if with_db else None
    ops.split_colsum(g, rows, cols, am, out.t, db.t if db else None, db0 is not None)
    return out, sinv, db


@pytest.mark.parametrize("cols", R.COLSUM_COLS)
@pytest.mark.parametrize("rows", R.COLSUM_ROWS)
def test_fusion_split_forms_split_colsum(rows, cols):
    mags = R.COLSUM_MAGS + ((0.0,) if (rows, cols) == (200, 96) else ())
    for mag in mags:
        what = f"split_colsum {rows}x{cols} mag={mag:g}"
        g_h, db0_h = R.colsum_inputs(rows, cols, mag)
        g, db0 = g_h.to(dev()), db0_h.to(dev())
        top = np.float32(float(g_h.abs().max()))
        am = torch.tensor([float(top)], device=dev())
        scale = R.sp_scale_for(top)
        out, sinv, db = colsum_run(g, rows, cols, am)
        got_sinv = sinv.intact("out_sinv").cpu().numpy()[0]
        print(f"{TAG} {what} scale: out_sinv {got_sinv!r} (host {np.float32(1.0 / scale)!r})")
        assert got_sinv.view(np.uint32) == np.float32(1.0 / scale).view(np.uint32)
        relabelled(held_sp, out, g_h.numpy() * np.float32(scale), what + " pieces")
        col = g_h.double().sum(0)
        r = bound_ratio(db.intact(what + " db"), col, R.colsum_bound(g_h))
        print(f"{TAG} {what} db: largest error at {r:.3e} of (ceil(rows/64) + 64) 2^-24 sum |g|")
        assert r <= 1.0
        _, _, db_acc = colsum_run(g, rows, cols, am, db0)
        r = bound_ratio(db_acc.intact(what + " db accumulate"), col + db0_h.double(), R.colsum_bound(g_h, db0_h))
        print(f"{TAG} {what} db accumulate: largest error at {r:.3e} of (ceil(rows/64) + 64) 2^-24 (sum |g| + |db0|)")
        assert r <= 1.0
        out2, sinv2, db2 = colsum_run(g, rows, cols, am)
        out3, sinv3, _ = colsum_run(g, rows, cols, am, with_db=False)
        again = (torch.equal(out2.intact("pieces").view(torch.int16), out.t.view(torch.int16)) and same_bits(db2.intact("db"), db.t)
                 and same_bits(sinv2.intact("sinv"), sinv.t))
        no_db = torch.equal(out3.intact("pieces").view(torch.int16), out.t.view(torch.int16)) and same_bits(sinv3.intact("sinv"), sinv.t)
        print(f"{TAG} {what} reruns: a second run gives the same bits {again}, a run without db the same pieces and 2^-k {no_db}")
        assert again and no_db
        if mag == 0.0:
            assert got_sinv == 1.0 and not u16(out.t).any() and not bits32(db.t).any(), "an all-zero g: scale 1, zero pieces, zero sums"


# ---------------------------------------------------------------- absmax_multi
def test_fusion_split_forms_absmax_multi():
    vs = [v.to(dev()) for v in R.absmax_tensors()]
    n = len(vs)
    want = [np.float32(float(v[:c].abs().max())) if c else np.float32(0) for v, c in zip(R.absmax_tensors(), R.ABSMAX_COUNTS)]
    ptrs = (C.c_void_p * n)(*[v.data_ptr() for v in vs])
    cnts = (C.c_int64 * n)(*R.ABSMAX_COUNTS)

    def launch(init):
        slots = Guarded((n,), init=torch.tensor(init, dtype=torch.float32))
        outs = (C.c_void_p * n)(*[slots.t[i:i + 1].data_ptr() for i in range(n)])
        from rot_mvgaze_amd._lib import check
        check(L().mvg_absmax_multi(ptrs, cnts, outs, n, st()), "absmax_multi")
        return bits32(slots.intact("absmax_multi slots"))

    first = [3.25] + [0.0] * (n - 1)                      # the zero-count tensor's slot must stay what it was
    got = launch(first)
    expect = np.array([np.float32(3.25)] + want[1:], dtype=np.float32).view(np.uint32)
    for i in range(n):
        print(f"{TAG} absmax_multi n={R.ABSMAX_COUNTS[i]} one-launch-of-8: slot {int(got[i]):#010x} (host {int(expect[i]):#010x})")
    assert (got == expect).all()
    assert got[6] == 0 and R.ABSMAX_COUNTS[5] > R.ABSMAX_GRID
    higher = [float(np.float32(2.0) * max(w, np.float32(1.0))) for w in want]
    got = launch(higher)
    kept = bool((got == np.array(higher, dtype=np.float32).view(np.uint32)).all())
    print(f"{TAG} absmax_multi higher-slots one-launch-of-8: slots pre-set above their maxima unchanged {kept}")
    assert kept


# ---------------------------------------------------------------- fuse_build_split
@pytest.mark.parametrize("rel", [True, False], ids=["rel", "no_rel"])
@pytest.mark.parametrize("which", ["xf", "xh", "both"])
@pytest.mark.parametrize("size", R.BUILD_SIZES, ids=lambda s: f"cf{s[0]}_nvec{s[1]}")
def test_fusion_split_forms_fuse_build_split(size, which, rel):
    from rot_mvgaze_amd import ops
    cf, nvec, mag = size
    pb = R.build_inputs(cf, nvec, mag)
    rows, c8i = pb.rows, cf // 8
    what = f"fuse_build_split cf={cf},nvec={nvec} {which},{'rel' if rel else 'no_rel'}"
    img, F = pb.img.to(dev()), pb.F.to(dev())
    am_i, am_f = torch.tensor([float(pb.am_img)], device=dev()), torch.tensor([float(pb.am_feat)], device=dev())
    sf_s, sh_s = slot(), slot()
    xf = sp_out(rows, cf + 3 * nvec, sf_s) if which != "xh" else None
    xh = sp_out(rows, cf + 3 * nvec, sh_s) if which != "xf" else None
    ops.fuse_build_split(img, F, pb.rel.to(dev()) if rel else None, pb.row_img.to(dev()), pb.partner.to(dev()), pb.ident.to(dev()),
                         xf.t if xf else None, xh.t if xh else None, am_i, am_f, rows, cf, nvec)
    img_rows = pb.img.numpy()[pb.row_img.long().numpy()]
    for name, out, sl, scale in (("xf", xf, sf_s, pb.sf), ("xh", xh, sh_s, pb.sh)):
        if out is None:
            continue
        got_sinv = sl.intact(name + " sinv").cpu().numpy()[0]
        print(f"{TAG} {what} {name} scale: sinv {got_sinv!r} (host {np.float32(1.0 / scale)!r})")
        assert got_sinv.view(np.uint32) == np.float32(1.0 / scale).view(np.uint32), f"{what}: {name}'s 2^-k"
        pieces = out.intact(f"{what} {name}")
        relabelled(held_sp, pieces[:, :c8i], img_rows * np.float32(scale), f"{what} {name} image columns")
        if name == "xh" or not rel:
            src = pb.ident if name == "xh" else pb.partner
            relabelled(held_sp, pieces[:, c8i:], pb.F.numpy()[src.long().numpy()] * np.float32(scale), f"{what} {name} copied feature columns")
        else:
            want, absterms = pb.rotated(True)
            back = R.sp_merge(u16(pieces[:, c8i:])).astype(np.float64) / scale
            r = bound_ratio(torch.from_numpy(back), want, R.build_bound(want, absterms, 1.0 / scale))
            print(f"{TAG} {what} {name} rotated columns: largest error at {r:.3e} of 3 2^-24 sum |r f| + 2^-23 |want| + 2^-25 2^-k")
            assert r <= 1.0


# ---------------------------------------------------------------- fuse_unbuild
@pytest.mark.parametrize("case", R.unbuild_cases(), ids=lambda c: "v%d_b%d_cf%d_nvec%d_%s_%s_%s" % (c[:5] + ("rel" if c[5] else "no_rel", "acc" if c[6] else "fresh")))
def test_fusion_split_forms_fuse_unbuild(case):
    from rot_mvgaze_amd import ops
    V, B, cf, nvec, mode, rel, accumulate = case
    uc = R.UnbuildCase(*case)
    what = "fuse_unbuild v%d,b%d,cf%d,nvec%d %s,%s,%s" % (V, B, cf, nvec, mode, "rel" if rel else "no_rel", "accumulate" if accumulate else "fresh")
    d_ = lambda t: t.to(dev()) if t is not None else None
    dxh, dxn, relm = d_(uc.dxh), d_(uc.dxn), d_(uc.rel)
    seg, vi = torch.tensor(uc.seg, dtype=torch.int32, device=dev()), torch.tensor(uc.vi, dtype=torch.int32, device=dev())
    outs = []
    for with_slot in (True, False):
        dF, da, am = Guarded((uc.S * B, 3 * nvec)), Guarded((V, B, cf), init=uc.da0 if accumulate else None), slot()
        ops.fuse_unbuild(dxh, dxn, relm, seg, vi, dF.t, da.t, accumulate, uc.S, V, uc.D, B, cf, nvec, absmax=am.t if with_slot else None)
        outs.append((dF.intact(what + " dF"), da.intact(what + " da"), am))
    dF, da, am = outs[0]
    rf = bound_ratio(dF.view(uc.S, B, 3, nvec), uc.dF, uc.dF_bound.expand_as(uc.dF))
    ra = bound_ratio(da, uc.da, uc.da_bound.expand_as(uc.da))
    print(f"{TAG} {what}: dF at {rf:.3e} and da at {ra:.3e} of terms x 2^-24 x sum |terms|")
    assert rf <= 1.0 and ra <= 1.0
    slot_holds_max(am, dF, what + " dF")
    same = torch.equal(outs[1][0], dF) and torch.equal(outs[1][1], da) and not bits32(outs[1][2].intact("unused slot")).any()
    print(f"{TAG} {what} absmax=None: the same dF and da, the slot untouched {same}")
    assert same


def test_fusion_split_forms_union_of_guarded_forms():
    """Runs last: what the guards above recorded is the whole table - all eight Linear instantiations and all seven tiles."""
    lin = sorted(f[1:] for f in _seen if f[0] == "linear")
    wg = sorted(f[1:] for f in _seen if f[0] == "wgrad")
    print(f"{TAG} forms seen: {len(lin)} Linear instantiations (bn, stages, dgrad) {lin}; {len(wg)} weight-gradient tiles {wg}")
    assert _seen == R.FORMS, f"never run: {sorted(R.FORMS - _seen, key=str)}; not in the table: {sorted(_seen - R.FORMS, key=str)}"
