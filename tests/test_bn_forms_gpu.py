"""Every pass and launch form of the BatchNorm kernels (csrc/bn.hip) at kernel level, against float64.

Which merge mvg_bn_finalize runs, how often a lane of a streaming pass loops and whether it changes channels on the way, and how
the reduce-type passes cut rows into chunks are host decisions (finalize_plan, stream_geometry, reduce_geometry / bwd_chunks from
the CUs the planners may use).  Every case FIRST asserts through the host-only plan query (mvg_bn_plan_query: answered by those
functions) the form it is about to run; ops.set_reserved_cus() moves chunk counts where that is cheaper than a larger shape.
FORMS below is the table of what must have run; the last test asserts the union of the guards' answers equals it.

Outputs start as NaN; so does every buffer the ops faces allocate for a launch (the partial workspace of the reduce passes) and
the stream's registered scratch (0xFF bytes) before a finalize: a slot a launch reads without having written it shows.

References (tests/bn_forms_ref.py; tests/test_bn_forms_cpu.py checks them against PyTorch's BatchNorm on CPU):
  finalize    the conv epilogue's fp32 partials written by the restatement from real fp32 rows, merged in float64; and the rows'
              own float64 statistics
  the passes  float64 formulas on the kernels' own fp32 inputs (mean, invstd, scale, shift), the ReLU pattern taken from the
              kernel's forward (an element within fp32 rounding of 0 may fall on either side); the stem tail by autograd
  exact       g = 1, no mask, integer y, integer mean, invstd = 1: every sum is an integer below 2^24, so s1 must EQUAL the row
              count, s2 the integer sum and dz_out g - one row dropped or counted twice cannot hide behind a tolerance

Bars (the project's, or bounded by the arithmetic - none fitted to the kernels):
  finalize vs the float64 merge of the same partials: mean, invstd, scale within 2 fp32 ulp (float64 arithmetic rounded once;
  scale one more fp32 product); shift within 2^-22 (|beta| + |mean scale|); the running statistics within 4 ulp per group of
  the fp32 recurrence, the ulp taken at the largest magnitude the recurrence mixes (a convex combination of the start value and
  the groups' statistics).  finalize vs the rows' own float64 statistics (well-conditioned set): test_bf16_gpu.py's 1e-4.
  Everything else: test_kernels_gpu.close() at test_bn_apply_and_backward's values (2e-5 forward and residual gradient, 1e-4
  sums and dy), test_eval_backward_gpu.py's 1e-6 for the eval-mode kernels, OUT_RTOL for bf16 outputs, sp_close / 1e-6 / 2^-22
  of the maximum for sp outputs against the fp32 kernels as tests/test_split_gpu.py has them, and bit-equality where today's
  tests assert it (mask sources, bf16 = rounded fp32, fused = unfused stem forward, sp sums = fp32 sums).

Every comparison prints `BN-FORMS <case> <form>: rel-L2 ...` (finalize: the largest error in its bar's units) before it
asserts.  Measured on an MI355X (profiles/bn_forms_errors.txt):
  finalize vs the float64 merge, every form: mean and invstd <= 0.50 ulp, scale <= 1.31 ulp, shift <= 0.71 of its bound, the
  running statistics <= 0.94 ulp per group; vs the rows' own statistics <= 5.4e-08
  apply / bwd-apply, second trip, with and without a channel step, three groups (relative L2 against float64):
      fp32 2.5e-08 .. 5.2e-08    sp 4.9e-08 .. 6.8e-08 (3.7e-08 .. 8.9e-08 against the fp32 kernel)    bf16 outputs 1.7e-03
  bwd-reduce and its split form, eval-bwd, every chunking and mask source: sums 5.7e-08 .. 1.3e-07, eval dy 4.2e-08 .. 4.6e-08
  stem tail: fp32 and sp 5.6e-09 .. 1.4e-07, bf16 outputs 1.5e-03 .. 1.9e-03
  506 comparisons are bit-equalities (mask sources, bf16 = rounded fp32, in-place forms, the exact counts).
Before the finalize kernels summed the partials around a pivot, the constant channels of the `constant` set (value -1234.567:
mean^2 / eps = 1.5e11) missed the 2-ulp bar by up to 796 ulp of invstd in every form: float64 rounding of sum s^2 / cnt - S mean.
"""
import contextlib
import ctypes as C
from unittest import mock

import pytest
import torch

import bn_forms_ref as ref
from bn_forms_ref import (ALL_GROUPS, BF16, ELEM_NAMES, EPS, FINALIZE_CASES, FP32, MOMENTUM, PER_GROUP, REDUCE_CASES, ROWS_PER_PARTIAL, SP,
                          STEM_CASES, STREAM_CASES, WALK_GROUPS)
from test_bf16_gpu import OUT_RTOL
from test_eval_backward_gpu import KTOL
from test_kernels_gpu import RTOL, close, dev
from test_split_gpu import sp_close

pytestmark = pytest.mark.gpu

NAN = float("nan")
SUMS_RTOL = 1e-4          # test_bn_apply_and_backward: dgamma, dbeta, dy
STATS_RTOL = 1e-4         # test_bf16_gpu.py: "bn mean" / "bn invstd" against the data's own float64 statistics

# (pass, element kind, what the query answered) - see guard_*() for the vocabulary
FORMS = {
    # finalize: merge form, sliced or not, scratch registered for the stream or not
    ("finalize", "walk-groups", "unsliced", "scratch"), ("finalize", "walk-groups", "sliced", "scratch"),
    ("finalize", "all-groups", "unsliced", "scratch"), ("finalize", "all-groups", "sliced", "scratch"),
    ("finalize", "per-group", "unsliced", "scratch"), ("finalize", "per-group", "sliced", "scratch"),
    ("finalize", "all-groups", "unsliced", "no-scratch"), ("finalize", "walk-groups", "unsliced", "no-scratch"),
    # streaming passes: loop trips of the busiest lane, whether a lane changes columns per trip, more than one group
    *[(p, e, t) for p in ("apply", "bwd-apply") for e in ("fp32", "bf16", "sp") for t in ("2-trips", "2-trips+step", "1-trip+groups")],
    # reduce-type passes over [rows][c]
    # (sp: the split reduce): what set the chunk count, chunks without rows, column blocks, a partly masked last block
    *[(p, e, t) for p, e in (("bwd-reduce", "fp32"), ("bwd-reduce", "bf16"), ("bwd-reduce", "sp"), ("eval-bwd", "fp32"))
      for t in ("cu-bound+empty-chunks", "one-chunk", "row-floor", "cu-bound")],
    *[(p, e, t) for p, e in (("bwd-reduce", "fp32"), ("bwd-reduce", "sp"), ("eval-bwd", "fp32")) for t in ("column-blocks", "column-blocks+masked-block")],
    # stem tail
    *[("pool-bwd-reduce", e, t) for e in ("fp32", "bf16", "sp") for t in ("one-chunk", "lines-per-chunk", "line-per-chunk")],
    ("pool-eval-bwd", "fp32", "one-workgroup"), ("pool-eval-bwd", "fp32", "workgroups"), ("pool-eval-bwd", "fp32", "workgroups+2-trips"),
}
_seen = set()


# ---------------------------------------------------------------- plumbing
def rel_l2(got, want):
    want = want.double().cpu()
    return ((got.double().cpu() - want).norm() / (want.norm() + 1e-300)).item()


def held(got, want, rtol, what):
    """Print the relative L2 error, then hold `got` to close() at rtol."""
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values (an element no lane wrote, or a stale workspace slot)"
    print(f"BN-FORMS {what}: rel-L2 {rel_l2(got, want):.3e}")
    close(got.float(), want, rtol, what)


def same(got, want, what):
    print(f"BN-FORMS {what}: rel-L2 {rel_l2(got.float(), want.float()):.3e} (bit-equal required)")
    assert torch.equal(got, want), what


@contextlib.contextmanager
def cus_left(n):
    """Leave n CUs to the planners (0: all of them)."""
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import lib
    total = lib().mvg_device_cus()
    assert total == 256, "the case tables are written for 256 CUs"
    try:
        ops.set_reserved_cus(total - n if n else 0)
        yield
    finally:
        ops.set_reserved_cus(0)


class _PoisoningTorch:
    """torch, for rot_mvgaze_amd.ops only: every buffer a face allocates for its launch (torch.empty) starts as NaN / 0xFF."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def empty(*a, **k):
        t = torch.empty(*a, **k)
        return t.fill_(NAN) if t.is_floating_point() else t.fill_(0xFF)


@contextlib.contextmanager
def poisoned_workspaces():
    from rot_mvgaze_amd import ops
    with mock.patch.object(ops, "torch", _PoisoningTorch()):
        yield


def poison_scratch():
    """0xFF over the current stream's registered workspace (registering it first, as the first launch would); its floats."""
    from rot_mvgaze_amd import ops
    handle = ops._s(True)
    ws = ops._workspaces[(torch.cuda.current_device(), handle)]
    ws.fill_(0xFF)
    return ws.numel() // 4


def nans(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=dev())


def sp_nans(*shape):
    from rot_mvgaze_amd import ops
    return ops.sp_empty(*shape, device=dev()).fill_(NAN)


def bf(x):
    return x.to(torch.bfloat16)


def store(x, elem):
    """A host fp32 tensor as the element kind's device tensor (sp passes read fp32)."""
    return (bf(x) if elem == BF16 else x).to(dev()).contiguous()


def values(x, elem):
    """The values the kernels see: bf16 storage rounds the inputs."""
    return bf(x).float() if elem == BF16 else x


# ---------------------------------------------------------------- guards
def guard_finalize(G, P, Cc, scratch_floats):
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import BN_PASS_FINALIZE
    pl = ops.bn_plan_query(BN_PASS_FINALIZE, FP32, G, P * ROWS_PER_PARTIAL, Cc, partials=P, scratch_floats=scratch_floats)
    got = tuple(pl[k] for k in ("form", "lanes_per_group", "slices", "partials_per_slice"))
    assert got == FINALIZE_CASES[(G, P, Cc, scratch_floats > 0)], f"finalize {G} x {P}: the plan moved this case to {got}"
    assert pl["scratch_floats"] <= scratch_floats or not scratch_floats
    _seen.add(("finalize", {WALK_GROUPS: "walk-groups", ALL_GROUPS: "all-groups", PER_GROUP: "per-group"}[pl["form"]],
               "sliced" if pl["slices"] else "unsliced", "scratch" if scratch_floats else "no-scratch"))
    return pl


def guard_stream(name, elem, G, rows, Cc):
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import BN_PASS_APPLY, BN_PASS_BWD_APPLY
    for p, pname in ((BN_PASS_APPLY, "apply"), (BN_PASS_BWD_APPLY, "bwd-apply")):
        pl = ops.bn_plan_query(p, elem, G, rows, Cc)
        got = (pl["accesses_per_group"], pl["grid_x"], pl["trips"], pl["step"])
        assert got == STREAM_CASES[(name, elem, G, rows, Cc)], f"{pname} {name} {ELEM_NAMES[elem]}: the plan moved this case to {got}"
        tag = "%d-trip%s" % (pl["trips"], "s" if pl["trips"] > 1 else "") + ("+step" if pl["step"] and pl["trips"] > 1 else "") + ("+groups" if G > 1 else "")
        _seen.add((pname, ELEM_NAMES[elem], tag))


def guard_reduce(bn_pass, elem, G, rows, Cc, cus):
    """Inside cus_left(cus).  elem SP: the split reduce (fp32 storage, a third workspace row)."""
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import BN_PASS_BWD_REDUCE
    pl = ops.bn_plan_query(bn_pass, elem, G, rows, Cc)
    got = tuple(pl[k] for k in ("cwn", "cw", "column_blocks", "row_lanes", "chunks", "rows_per_chunk", "empty_chunks"))
    assert got == REDUCE_CASES[(G, rows, Cc, cus)][BF16 if elem == BF16 else FP32], f"reduce {(G, rows, Cc, cus)}: the plan moved this case to {got}"
    tags = []
    if pl["chunks"] == 1:
        tags.append("one-chunk")
    elif pl["chunks"] < -(-rows // 64):
        tags.append("cu-bound")
    if pl["empty_chunks"]:
        tags.append("empty-chunks")
    if pl["column_blocks"] > 1:
        tags.append("column-blocks")
    if pl["cwn"] % pl["cw"]:
        tags.append("masked-block")
    _seen.add(("bwd-reduce" if bn_pass == BN_PASS_BWD_REDUCE else "eval-bwd", ELEM_NAMES[elem], "+".join(tags) or "row-floor"))
    return pl


def guard_stem(elem, case, train):
    """Inside cus_left(case's CUs)."""
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import BN_PASS_POOL_BWD_REDUCE, BN_PASS_POOL_EVAL_BWD
    G, N, H, W, Cc, cus = case
    want_train, want_eval = STEM_CASES[case]
    if train:
        pl = ops.bn_plan_query(BN_PASS_POOL_BWD_REDUCE, elem, G, 0, Cc, N, H, W)
        assert (pl["chunks"], pl["rows_per_chunk"]) == want_train, f"stem {case}: the plan moved this case to {pl}"
        tag = "one-chunk" if pl["chunks"] == 1 else "line-per-chunk" if pl["rows_per_chunk"] == 1 else "lines-per-chunk"
        _seen.add(("pool-bwd-reduce", ELEM_NAMES[elem], tag))
    else:
        pl = ops.bn_plan_query(BN_PASS_POOL_EVAL_BWD, elem, G, 0, Cc, N, H, W)
        assert pl["chunks"] == want_eval, f"stem {case}: the plan moved this case to {pl}"
        items = N * ((H + 1) // 2) * ((W + 1) // 2) * (Cc // 4)
        tag = "one-workgroup" if pl["chunks"] == 1 else "workgroups" + ("+2-trips" if items > pl["chunks"] * 256 else "")
        _seen.add(("pool-eval-bwd", ELEM_NAMES[elem], tag))
    return pl


# ---------------------------------------------------------------- finalize
def _finalize_launch(stats, G, P, rows, Cc, gamma, beta, rm, rv, outs, scratch):
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import lib
    if scratch:
        poison_scratch()
        ops.bn_finalize(stats, G, P, ROWS_PER_PARTIAL, rows, Cc, gamma, beta, rm, rv, MOMENTUM, EPS, *outs)
    else:
        side = torch.cuda.Stream()                           # a stream nobody registered a workspace for
        side.wait_stream(torch.cuda.current_stream())
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)
        mean, invstd, scale, shift = outs
        with torch.cuda.stream(side):
            rc = lib().mvg_bn_finalize(ptr(stats), G, P, ROWS_PER_PARTIAL, rows, Cc, ptr(gamma), ptr(beta), ptr(rm), ptr(rv),
                                       C.c_float(MOMENTUM), C.c_float(EPS), ptr(mean), ptr(invstd), ptr(scale), ptr(shift),
                                       C.c_void_p(side.cuda_stream))
        assert rc == 0
        side.synchronize()
    torch.cuda.synchronize()


@pytest.mark.parametrize("G,P,Cc,scratch", list(FINALIZE_CASES), ids=["g%d_p%d_c%d_%s" % (g, p, c, "scratch" if sc else "no-scratch") for g, p, c, sc in FINALIZE_CASES])
def test_finalize_every_merge_form_against_the_float64_merge(G, P, Cc, scratch):
    from rot_mvgaze_amd._lib import lib
    pl = guard_finalize(G, P, Cc, lib().mvg_scratch_bytes() // 4 if scratch else 0)
    form = f"g{G}_p{P}_c{Cc} form{pl['form']}{'/sliced' if pl['slices'] else ''}{'' if scratch else '/no-scratch'}"
    gamma, beta, rm0, rv0 = ref.finalize_params(Cc)
    gd, bd = gamma.to(dev()), beta.to(dev())
    for kind, rows_name, with_running in ref.finalize_runs(G, P):
        stats, rows, want = ref.finalize_reference(G, P, Cc, kind, rows_name, with_running)
        assert bool(torch.isnan(stats).any()) == (rows_name in ("surplus", "one-row", "one-over")), "surplus slots hold NaN"
        rm, rv = (rm0.to(dev()), rv0.to(dev())) if with_running else (None, None)
        outs = [nans(G, Cc) for _ in range(4)]
        _finalize_launch(stats.to(dev()), G, P, rows, Cc, gd, bd, rm, rv, outs, scratch)
        mean, invstd, scale, shift = (t.cpu() for t in outs)
        what = f"{form} {kind}/{rows_name}{'' if with_running else '/no-running'}"
        assert all(bool(torch.isfinite(t).all()) for t in (mean, invstd, scale, shift)), f"{what}: NaN (a surplus partial or a stale slot was read)"
        u = {k: ref.ulps(t, want[k]) for k, t in (("mean", mean), ("invstd", invstd), ("scale", scale))}
        sh_bound = 2.0 ** -22 * (beta.double().abs()[None] + (want["mean"] * want["scale"]).abs())
        sh = float(((shift.double() - want["shift"]).abs() / sh_bound).max())
        line = f"BN-FORMS finalize {what}: rel-L2 mean {rel_l2(mean, want['mean']):.3e} invstd {rel_l2(invstd, want['invstd']):.3e}; ulp " \
               f"mean {u['mean']:.2f} invstd {u['invstd']:.2f} scale {u['scale']:.2f}; shift {sh:.3f} of its bound"
        r_err = {}
        if with_running:
            for key, got, start, stat in (("rm", rm, rm0, want["mean"]), ("rv", rv, rv0, want["unbiased"])):
                mag = torch.maximum(start.double().abs(), stat.abs().amax(0))          # what the recurrence mixes
                r_err[key] = float(((got.cpu().double() - want[key].double()).abs() / (mag * 2.0 ** -23)).max())
            line += f"; running mean {r_err['rm']:.2f} var {r_err['rv']:.2f} ulp (bar {4 * G})"
        print(line)
        assert max(u.values()) <= 2.0, f"{what}: {u} fp32 ulp from the float64 merge of the same partials"
        assert sh <= 1.0, f"{what}: shift off by {sh:.3f} x 2^-22 (|beta| + |mean scale|)"
        for key, e in r_err.items():
            assert e <= 4 * G, f"{what}: {key} {e:.2f} ulp from the fp32 recurrence in group order (bar {4 * G})"
        if kind == "well":                                    # ... and the rows' own statistics, at the project's bar
            dm, di = ref.group_stats(ref.finalize_data(G, P, Cc, kind)[:, :rows])
            held(mean, dm, STATS_RTOL, f"finalize {what} mean vs the rows")
            held(invstd, di, STATS_RTOL, f"finalize {what} invstd vs the rows")
        if kind == "constant":
            assert float((invstd[:, :4].double() - EPS ** -0.5).abs().max()) <= 1e-3 * EPS ** -0.5, "variance 0: invstd = 1 / sqrt(eps)"


# ---------------------------------------------------------------- streaming passes
def _unit(elem, G, rows, Cc, seed):
    """Inputs of one unit, host fp32 (as the kernels see them) and device storage."""
    y = values(ref.randn((G, rows, Cc), seed) * 2 + 0.5, elem)
    r = values(ref.randn((G, rows, Cc), seed + 1), elem)
    go = values(ref.randn((G, rows, Cc), seed + 2), elem)
    gamma, beta = ref.randn((Cc,), seed + 3) * 0.2 + 1, ref.randn((Cc,), seed + 4) * 0.2
    gamma[::5] *= -1
    m64, i64 = ref.group_stats(y)
    mean, invstd = m64.float(), i64.float()
    scale = gamma[None] * invstd                              # fp32, as the finalize kernel forms them
    shift = beta[None] - mean * scale
    return dict(y=y, r=r, go=go, gamma=gamma, beta=beta, mean=mean, invstd=invstd, scale=scale, shift=shift)


def _apply(elem, u, G, rows, Cc, residual, res_affine, relu, bits, out_sinv=None, res_sp_scale=None):
    """One forward launch in the element kind's storage; returns (output as fp32 values, mask bytes or None).  sp: residual
    fp32 (raw) or, with res_sp_scale, an sp identity stored times that power of two; out_sinv: the output's 2^-k."""
    from rot_mvgaze_amd import ops
    d = lambda t: None if t is None else t.to(dev())
    yd, sc, sh = store(u["y"], elem), d(u["scale"]), d(u["shift"])
    ra = None if res_affine is None else (d(res_affine[0]), d(res_affine[1]))
    if elem == SP:
        out = sp_nans(G, rows, Cc)
        if out_sinv is not None:
            out.sinv = torch.full((1,), out_sinv, device=dev())
        rd = None if residual is None else (ops.split_f32(d(residual), res_sp_scale) if res_sp_scale else d(residual))
        b = ops.bn_apply_split(yd, sc, sh, rd, relu, out, G, rows, Cc, ra, want_bits=bits)
        return ops.merge_sp(out).cpu(), (b.cpu() if bits else None)
    out = nans(G, rows, Cc, dtype=yd.dtype)
    rd = None if residual is None else store(residual, elem)
    if bits:
        assert relu
        return out, ops.bn_apply_bits(yd, sc, sh, rd, out, G, rows, Cc, ra).cpu()
    ops.bn_apply(yd, sc, sh, rd, relu, out, G, rows, Cc, ra)
    return out, None


@pytest.mark.parametrize("name,elem,G,rows,Cc", list(STREAM_CASES), ids=["%s-%s-g%d_r%d_c%d" % (n, ELEM_NAMES[e], g, r, c) for n, e, g, r, c in STREAM_CASES])
def test_streaming_passes_every_epilogue(name, elem, G, rows, Cc):
    """bn_apply / bn_bwd_apply (fp32, bf16) and their sp forms: the loop's second trip with the lane keeping (step == 0) or
    changing (step != 0) its channels, three groups; every epilogue the entry points offer."""
    from rot_mvgaze_amd import ops
    guard_stream(name, elem, G, rows, Cc)
    if Cc == 96:                                              # streams, but does not reduce: s1 / s2 come from the reference
        g0 = nans(1, 8, 96)
        with pytest.raises(RuntimeError, match=ref.REDUCE_REJECTED):
            ops.bn_bwd_reduce(g0, None, g0, nans(1, 96), nans(1, 96), 1, 8, 96, nans(1, 96), nans(1, 96), nans(96), nans(96), False)
    u = _unit(elem, G, rows, Cc, 100 * Cc + G)
    tag = f"{name} {ELEM_NAMES[elem]} g{G}_r{rows}_c{Cc}"
    out_rtol = OUT_RTOL if elem == BF16 else RTOL
    fp32_u = u                                                # the fp32 kernels on the same values: bf16 = rounded fp32, sp = fp32 to the last bit
    d = lambda t: None if t is None else t.to(dev())
    rs, rh = ref.randn((G, Cc), 7) * 0.2 + 1, ref.randn((G, Cc), 8) * 0.2
    epilogues = [("plain+relu", None, None, True, False), ("residual+relu+bits", u["r"], None, True, True),
                 ("raw-residual+affine", u["r"], (rs, rh), False, False), ("residual", u["r"], None, False, False)]
    outs = {}
    for ep, res, raff, relu, bits in epilogues:
        want = ref.apply_ref(u["y"], u["scale"], u["shift"], res, raff, relu)[1]
        got, b = _apply(elem, u, G, rows, Cc, res, raff, relu, bits)
        outs[ep] = got                                         # (sp: replaced below by the fp32 kernel's, whose sign the mask bits record)
        held(got.float().cpu() if elem != SP else got, want, out_rtol, f"{tag} apply {ep}")
        if elem != FP32:
            f32, fb = _apply(FP32, fp32_u, G, rows, Cc, res, raff, relu, bits)
            if elem == BF16:
                same(got, bf(f32), f"{tag} apply {ep} == the rounded fp32 output")
            else:
                outs[ep] = f32.cpu()
                print(f"BN-FORMS {tag} apply {ep} vs the fp32 kernel: rel-L2 {rel_l2(got, f32):.3e} (sp_close)")
                sp_close(got, f32.cpu(), f"{tag} apply {ep}")
        if bits:
            on = (got > 0) if elem != SP else (f32 > 0)         # sp: the bits come from the value before it is split
            same(b, ref.mask_bytes(on.cpu(), 8 if elem == BF16 else 4), f"{tag} apply {ep} mask bytes")
            plain, _ = _apply(elem, u, G, rows, Cc, res, raff, True, False)
            same(plain, got, f"{tag} apply {ep} == without the bits")
    if elem == SP:
        # the scaled output (stored times 2^3) and an sp identity that carries its own 2^-k
        want = ref.apply_ref(u["y"], u["scale"], u["shift"], u["r"], None, True)[1]
        f32, _ = _apply(FP32, u, G, rows, Cc, u["r"], None, True, False)
        got, _ = _apply(SP, u, G, rows, Cc, u["r"], None, True, False, out_sinv=0.125)
        held(got, want, RTOL, f"{tag} apply residual+relu scaled-output")
        sp_close(got, f32.cpu(), f"{tag} apply scaled output")
        rsp = ops.merge_sp(ops.split_f32(d(u["r"]), 4.0)).cpu()  # the identity's values after the split
        want = ref.apply_ref(u["y"], u["scale"], u["shift"], rsp, None, True)[1]
        got, _ = _apply(SP, u, G, rows, Cc, u["r"], None, True, False, res_sp_scale=4.0)
        held(got, want, RTOL, f"{tag} apply sp-identity+relu")
        f32, _ = _apply(FP32, dict(u, r=rsp), G, rows, Cc, rsp, None, True, False)
        sp_close(got, f32.cpu(), f"{tag} apply sp identity")

    # ---- backward apply: masks taken from the forward launches above
    yd, god = store(u["y"], elem), store(u["go"], elem)
    md, isd, gd = d(u["mean"]), d(u["invstd"]), d(u["gamma"])
    for ep, affine in (("residual+relu+bits", False), ("plain+relu", True), ("residual", None)):
        act = outs[ep]
        mask = None if affine is None else (act > 0).cpu()
        b = ref.train_bwd_ref(u["go"], u["y"], u["mean"], u["invstd"], u["gamma"], mask)
        s1, s2 = d(b["s1"].float()), d(b["s2"].float())
        relu_affine = (d(u["scale"]), d(u["shift"])) if affine else None
        if elem == SP:
            # the sp form takes the mask from y (relu_affine) or an already masked gradient, and mx from the reduce pass
            gin = god if affine is not False else d(b["dz"].float())
            mx = d(b["dz"].abs().amax(1).float())
            dy = sp_nans(G, rows, Cc)
            ops.bn_bwd_apply_split(gin, yd, md, isd, gd, s1, s2, G, rows, Cc, dy, relu_affine, mx)
            got = ops.merge_sp(dy).cpu()
            held(got, b["dy"], SUMS_RTOL, f"{tag} bwd-apply {ep}")
            want_f = nans(G, rows, Cc)
            ops.bn_bwd_apply(gin, None, yd, md, isd, gd, s1, s2, G, rows, Cc, want_f, None, relu_affine)
            e = float((got - want_f.cpu()).abs().max()) / float(want_f.abs().max())
            print(f"BN-FORMS {tag} bwd-apply {ep} vs the fp32 kernel: max error {e:.3e} of the maximum (bar 1e-6)")
            assert e <= 1e-6
            sinv, m = ref.dy_scale_inverse(u["gamma"], u["invstd"], b["s1"].float(), b["s2"].float(), b["dz"].abs().amax(1).float(), rows)
            ok = {sinv} | ({sinv * 2} if m > 1 - 1e-5 else set()) | ({sinv / 2} if m < 0.5 + 1e-5 else set())
            assert float(dy.sinv) in ok, f"{tag} bwd-apply {ep}: dy scale 2^{torch.log2(dy.sinv).item():.0f}, host evaluation {sinv}"
            assert float(dy.float().abs().max()) < 65504.0
            continue
        actd = None if affine is not False else act
        dy, dz = nans(G, rows, Cc, dtype=yd.dtype), nans(G, rows, Cc, dtype=yd.dtype)
        ops.bn_bwd_apply(god, actd, yd, md, isd, gd, s1, s2, G, rows, Cc, dy, dz, relu_affine)
        held(dy.float().cpu(), b["dy"], OUT_RTOL if elem == BF16 else SUMS_RTOL, f"{tag} bwd-apply {ep} dy")
        dz_want = b["dz"].float()
        same(dz.cpu(), bf(dz_want) if elem == BF16 else dz_want, f"{tag} bwd-apply {ep} dz_out")
        if affine:                                            # the mask rebuilt from y == the mask taken from the activation
            dy2 = nans(G, rows, Cc, dtype=yd.dtype)
            ops.bn_bwd_apply(god, act, yd, md, isd, gd, s1, s2, G, rows, Cc, dy2, None, None)
            same(dy2, dy, f"{tag} bwd-apply {ep}: mask from y == mask from act")
        # the aliased forms the backbone uses: dy in place of g; dz in place of g
        g2 = god.clone()
        ops.bn_bwd_apply(g2, actd, yd, md, isd, gd, s1, s2, G, rows, Cc, g2, None, relu_affine)
        held(g2.float().cpu(), b["dy"], OUT_RTOL if elem == BF16 else SUMS_RTOL, f"{tag} bwd-apply {ep} dy in place")
        g3, dy3 = god.clone(), nans(G, rows, Cc, dtype=yd.dtype)
        ops.bn_bwd_apply(g3, actd, yd, md, isd, gd, s1, s2, G, rows, Cc, dy3, g3, relu_affine)
        same(dy3, dy, f"{tag} bwd-apply {ep} dy with dz in place")
        same(g3, dz, f"{tag} bwd-apply {ep} dz in place")


# ---------------------------------------------------------------- reduce-type passes
REDUCE_PARAMS = [(case, elem) for case, per in REDUCE_CASES.items() for elem in (FP32, BF16) if per[elem] is not None]


def _reduce_inputs(elem, G, rows, Cc):
    from rot_mvgaze_amd import ops
    u = _unit(elem, G, rows, Cc, 10 * Cc + G + rows % 97)
    d = lambda t: t.to(dev())
    yd, sc, sh = store(u["y"], elem), d(u["scale"]), d(u["shift"])
    act_res = nans(G, rows, Cc, dtype=yd.dtype)
    bits = ops.bn_apply_bits(yd, sc, sh, store(u["r"], elem), act_res, G, rows, Cc)
    act_plain = nans(G, rows, Cc, dtype=yd.dtype)
    ops.bn_apply(yd, sc, sh, None, True, act_plain, G, rows, Cc)
    masks = {"bits": (act_res > 0).cpu(), "act": (act_res > 0).cpu(), "affine": (act_plain > 0).cpu(), "none": None}
    return u, yd, sc, sh, act_res, bits, masks


@pytest.mark.parametrize("case,elem", REDUCE_PARAMS, ids=["g%d_r%d_c%d_cus%d-" % c + ELEM_NAMES[e] for c, e in REDUCE_PARAMS])
def test_reduce_passes_every_mask_source_and_chunking(case, elem):
    """bn_bwd_reduce (fp32, bf16; the split form with mx and the dy scale) and bn_eval_bwd: empty trailing chunks, one chunk,
    the unrolled loop and its tail, a half-masked column block, the chunking under two CU budgets."""
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import BN_PASS_BWD_REDUCE, BN_PASS_EVAL_BWD
    G, rows, Cc, cus = case
    u, yd, sc, sh, act_res, bits, masks = _reduce_inputs(elem, G, rows, Cc)
    d = lambda t: t.to(dev())
    god, md, isd, gd = store(u["go"], elem), d(u["mean"]), d(u["invstd"]), d(u["gamma"])
    tag = f"{ELEM_NAMES[elem]} g{G}_r{rows}_c{Cc}_cus{cus}"
    rm_h, rv_h = ref.randn((Cc,), 21) * 0.5 + 0.5, ref.randn((Cc,), 22).abs() + 0.5
    with cus_left(cus), poisoned_workspaces():
        guard_reduce(BN_PASS_BWD_REDUCE, elem, G, rows, Cc, cus)
        res = {}
        for src, mask in masks.items():
            b = ref.train_bwd_ref(u["go"], u["y"], u["mean"], u["invstd"], u["gamma"], mask)
            s1, s2, dg, db = nans(G, Cc), nans(G, Cc), nans(Cc), nans(Cc)
            dz = nans(G, rows, Cc, dtype=yd.dtype)
            if src == "bits":
                ops.bn_bwd_reduce_bits(god, bits, yd, md, isd, G, rows, Cc, s1, s2, dg, db, False, dz_out=dz)
            else:
                ops.bn_bwd_reduce(god, act_res if src == "act" else None, yd, md, isd, G, rows, Cc, s1, s2, dg, db, False,
                                  (sc, sh) if src == "affine" else None, dz_out=dz)
            res[src] = (s1, s2, dg, db, dz)
            for name, got in (("s1", s1), ("s2", s2), ("dgamma", dg), ("dbeta", db)):
                held(got.cpu(), b[name], SUMS_RTOL, f"{tag} bwd-reduce train/{src} {name}")
            dz_want = b["dz"].float()
            same(dz.cpu(), bf(dz_want) if elem == BF16 else dz_want, f"{tag} bwd-reduce train/{src} dz_out")
            if elem == FP32:
                # the split form: the same sums, max |dz| per (group, channel), and the 2^-k of the dy its bound allows
                guard_reduce(BN_PASS_BWD_REDUCE, SP, G, rows, Cc, cus)
                t1, t2, tg, tb, mx, sinv = nans(G, Cc), nans(G, Cc), nans(Cc), nans(Cc), nans(G, Cc), nans(1)
                if src != "act":
                    ops.bn_bwd_reduce_split(god, bits if src == "bits" else None, yd, md, isd, G, rows, Cc, t1, t2, tg, tb, False, mx,
                                            (sc, sh) if src == "affine" else None, None, gd, sinv)
                    for name, got in (("s1", t1), ("s2", t2), ("dgamma", tg), ("dbeta", tb)):
                        held(got.cpu(), b[name], SUMS_RTOL, f"{tag} bwd-reduce split/{src} {name}")
                    same(mx.cpu(), b["dz"].abs().amax(1).float(), f"{tag} bwd-reduce split/{src} mx == max |dz|")
                    want, m = ref.dy_scale_inverse(u["gamma"], u["invstd"], t1.cpu(), t2.cpu(), mx.cpu(), rows)
                    ok = {want} | ({want * 2} if m > 1 - 1e-5 else set()) | ({want / 2} if m < 0.5 + 1e-5 else set())
                    assert float(sinv) in ok, f"{tag} split/{src}: dy_sinv {float(sinv)} but the host evaluates {want} (mantissa {m})"
        for k in range(5):                                    # the three mask sources of one unit: the same bits
            same(res["bits"][k], res["act"][k], f"{tag} bwd-reduce train bits == act [{k}]")
        if elem == FP32:
            guard_reduce(BN_PASS_EVAL_BWD, FP32, G, rows, Cc, cus)
            rmd, rvd = d(rm_h), d(rv_h)
            for src, mask in masks.items():
                e = ref.eval_bwd_ref(u["go"], u["y"], u["gamma"], rm_h, rv_h, EPS, mask)
                dy, dz, dg, db = nans(G, rows, Cc), nans(G, rows, Cc), nans(Cc), nans(Cc)
                kw = {"bits": dict(relu_bits=bits), "act": dict(act=act_res), "affine": dict(relu_affine=(sc, sh)), "none": {}}[src]
                ops.bn_eval_bwd(god, yd, gd, rmd, rvd, EPS, G, rows, Cc, dy, dg, db, False, dz_out=dz, **kw)
                held(dy.cpu(), e["dy"], KTOL, f"{tag} eval-bwd {src} dy")
                held(dg.cpu(), e["dgamma"], KTOL, f"{tag} eval-bwd {src} dgamma")
                held(db.cpu(), e["dbeta"], KTOL, f"{tag} eval-bwd {src} dbeta")
                same(dz.cpu(), e["dz"].float(), f"{tag} eval-bwd {src} dz_out")
                g2 = god.clone()                              # dy in place of g
                ops.bn_eval_bwd(g2, yd, gd, rmd, rvd, EPS, G, rows, Cc, g2, None, None, False, **kw)
                same(g2, dy, f"{tag} eval-bwd {src} dy in place")


@pytest.mark.parametrize("case,elem", REDUCE_PARAMS, ids=["g%d_r%d_c%d_cus%d-" % c + ELEM_NAMES[e] for c, e in REDUCE_PARAMS])
def test_reduce_passes_count_every_row_exactly_once(case, elem):
    """g = 1, no mask, integer y, integer mean, invstd = 1: s1 EQUALS the row count and s2 the integer sum of (y - mean) - all
    partial sums are integers below 2^24, exact in fp32 in any order - and dz_out is g."""
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import BN_PASS_BWD_REDUCE, BN_PASS_EVAL_BWD
    G, rows, Cc, cus = case
    gen = torch.Generator().manual_seed(rows + Cc)
    y = torch.randint(-8, 9, (G, rows, Cc), generator=gen).float()
    mean = torch.randint(-3, 4, (G, Cc), generator=gen).float()
    ones_gc, g = torch.ones(G, Cc), torch.ones(G, rows, Cc)
    s2_want = (y.double() - mean.double()[:, None]).sum(1)
    assert float(s2_want.abs().max()) < 2 ** 24 and G * rows * 11 < 2 ** 24
    d = lambda t: t.to(dev())
    yd, gd_ = store(y, elem), store(g, elem)
    tag = f"exact {ELEM_NAMES[elem]} g{G}_r{rows}_c{Cc}_cus{cus}"
    with cus_left(cus), poisoned_workspaces():
        guard_reduce(BN_PASS_BWD_REDUCE, elem, G, rows, Cc, cus)
        s1, s2, dg, db = nans(G, Cc), nans(G, Cc), nans(Cc), nans(Cc)
        dz = nans(G, rows, Cc, dtype=yd.dtype)
        ops.bn_bwd_reduce(gd_, None, yd, d(mean), d(ones_gc), G, rows, Cc, s1, s2, dg, db, False, None, dz_out=dz)
        same(s1.cpu(), torch.full((G, Cc), float(rows)), f"{tag} bwd-reduce s1 == rows")
        same(s2.cpu(), s2_want.float(), f"{tag} bwd-reduce s2")
        same(db.cpu(), torch.full((Cc,), float(G * rows)), f"{tag} bwd-reduce dbeta == groups x rows")
        same(dg.cpu(), s2_want.sum(0).float(), f"{tag} bwd-reduce dgamma")
        same(dz, gd_, f"{tag} bwd-reduce dz_out == g")
        if elem == FP32:
            guard_reduce(BN_PASS_BWD_REDUCE, SP, G, rows, Cc, cus)
            t1, t2, mx = nans(G, Cc), nans(G, Cc), nans(G, Cc)
            ops.bn_bwd_reduce_split(gd_, None, yd, d(mean), d(ones_gc), G, rows, Cc, t1, t2, None, None, False, mx)
            same(t1.cpu(), torch.full((G, Cc), float(rows)), f"{tag} bwd-reduce split s1 == rows")
            same(t2.cpu(), s2_want.float(), f"{tag} bwd-reduce split s2")
            same(mx.cpu(), ones_gc, f"{tag} bwd-reduce split mx == 1")
            # eval mode: running_var = 1 with eps = 0 makes invstd_r exactly 1; gamma = 2
            guard_reduce(BN_PASS_EVAL_BWD, FP32, G, rows, Cc, cus)
            rm = mean[0].contiguous()
            dy, dz2, dg, db = nans(G, rows, Cc), nans(G, rows, Cc), nans(Cc), nans(Cc)
            ops.bn_eval_bwd(gd_, yd, d(torch.full((Cc,), 2.0)), d(rm), d(torch.ones(Cc)), 0.0, G, rows, Cc, dy, dg, db, False, dz_out=dz2)
            same(db.cpu(), torch.full((Cc,), float(G * rows)), f"{tag} eval-bwd dbeta == groups x rows")
            same(dg.cpu(), (y.double() - rm.double()).sum((0, 1)).float(), f"{tag} eval-bwd dgamma")
            same(dy.cpu(), 2 * g, f"{tag} eval-bwd dy == gamma g")
            same(dz2, gd_, f"{tag} eval-bwd dz_out == g")


# ---------------------------------------------------------------- stem tail
def _winner_values(y_nhwc, am, H, W):
    """y at every pooling window's argmax pixel: am [G, N, ho, wo, C] holds kh * 3 + kw of the 3x3 / 2 / 1 window."""
    G, N, ho, wo, Cc = am.shape
    k = am.long()
    iy = 2 * torch.arange(ho)[None, None, :, None, None] - 1 + k // 3
    ix = 2 * torch.arange(wo)[None, None, None, :, None] - 1 + k % 3
    assert bool(((iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)).all()), "an argmax outside the image"
    flat = (iy * W + ix) * Cc + torch.arange(Cc)[None, None, None, None, :]
    return y_nhwc.reshape(G, N, H * W * Cc).gather(2, flat.reshape(G, N, -1)).reshape(am.shape), flat


@pytest.mark.parametrize("case", list(STEM_CASES), ids=lambda c: "g%d_n%d_%dx%d_c%d_cus%d" % c)
@pytest.mark.parametrize("elem", [FP32, BF16, SP], ids=lambda e: ELEM_NAMES[e])
def test_stem_tail_train_and_eval(case, elem):
    """mvg_bn_relu_maxpool_{fwd, bwd_reduce, bwd_apply} in every storage family and mvg_bn_relu_maxpool_eval_bwd against
    autograd through float64 batch_norm -> relu -> max_pool2d; negative gamma on some channels (the window order flips)."""
    from rot_mvgaze_amd import ops
    G, N, H, W, Cc, cus = case
    ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    rows = N * H * W
    tag = f"stem {ELEM_NAMES[elem]} g{G}_n{N}_{H}x{W}_c{Cc}_cus{cus}"
    y = values(ref.randn((G, N, Cc, H, W), 11 + H) * 1.5 + 0.2, elem)
    gamma, beta = ref.randn((Cc,), 12) * 0.3 + 1.0, ref.randn((Cc,), 13) * 0.3
    gamma[::7] *= -1
    gp_of = lambda shape: values(ref.randn(shape, 14), elem)
    nhwc = lambda t: t.permute(0, 1, 3, 4, 2).contiguous()
    d = lambda t: t.to(dev())
    y_nhwc = nhwc(y)
    yd, gd = store(y_nhwc, elem), d(gamma)
    st_f32 = torch.float32 if elem != BF16 else torch.bfloat16
    with cus_left(cus), poisoned_workspaces():
        for train in (True, False) if elem == FP32 else (True,):
            rm_h, rv_h = ref.randn((Cc,), 31) * 0.3 + 0.2, ref.randn((Cc,), 32).abs() + 0.8
            want = ref.stem_tail_ref(y, gamma, beta, gp_of, train, rm_h, rv_h)
            guard_stem(elem, case, train)
            if train:
                m64, i64 = ref.group_stats(y_nhwc.reshape(G, rows, Cc))
                mean, invstd = d(m64.float()), d(i64.float())
                scale = (gd[None] * invstd).contiguous()
                shift = (d(beta)[None] - mean * scale).contiguous()
            else:
                scale, shift = nans(G, Cc), nans(G, Cc)
                ops.bn_eval_affine(G, Cc, gd, d(beta), d(rm_h), d(rv_h), EPS, scale, shift)
            mode = "train" if train else "eval"
            am = torch.full((G, N, ho, wo, Cc), 0xFF, dtype=torch.uint8, device=dev())
            pooled_want = nhwc(want["pooled"])
            if elem == SP:
                pooled = sp_nans(G, N, ho, wo, Cc)
                ops.bn_relu_maxpool_fwd_split(yd, scale, shift, pooled, am, G, N, H, W, Cc, ho, wo)
                pf, amf = nans(G, N, ho, wo, Cc), torch.empty_like(am)
                ops.bn_relu_maxpool_fwd(yd, scale, shift, pf, amf, G, N, H, W, Cc, ho, wo)
                got = ops.merge_sp(pooled).cpu()
                sp_close(got, pf.cpu(), f"{tag} pooled map")
                same(am, amf, f"{tag} {mode} argmax sp == fp32")
            else:
                pooled = nans(G, N, ho, wo, Cc, dtype=st_f32)
                ops.bn_relu_maxpool_fwd(yd, scale, shift, pooled, am, G, N, H, W, Cc, ho, wo)
                got = pooled.float().cpu()
                if elem == FP32:                              # the unfused kernels give the same bits (same fma, same scan order)
                    a0 = nans(G, rows, Cc)
                    ops.bn_apply(yd, scale, shift, None, True, a0, G, rows, Cc)
                    p2, am2 = nans(G, N, ho, wo, Cc), torch.empty_like(am)
                    ops.maxpool_fwd(a0, p2, am2, G * N, H, W, Cc, ho, wo)
                    same(p2, pooled, f"{tag} {mode} fused == unfused forward")
            held(got, pooled_want, OUT_RTOL if elem == BF16 else 1e-5, f"{tag} {mode} forward")
            gpd = store(nhwc(want["gp"]), elem)
            dy_want = nhwc(want["dy"])
            if not train:
                dy, dg, db = nans(G, N, H, W, Cc), nans(Cc), nans(Cc)
                ops.bn_relu_maxpool_eval_bwd(gpd, am, yd, scale, shift, gd, d(rm_h), d(rv_h), EPS, G, N, H, W, Cc, ho, wo, dy, dg, db, False)
                held(dy.cpu(), dy_want, KTOL, f"{tag} eval dy")
                held(dg.cpu(), want["dgamma"], KTOL, f"{tag} eval dgamma")
                held(db.cpu(), want["dbeta"], KTOL, f"{tag} eval dbeta")
                continue
            s12, dg, db = nans(2, G, Cc), nans(Cc), nans(Cc)
            ops.bn_relu_maxpool_bwd_reduce(gpd, am, yd, mean, invstd, scale, shift, G, N, H, W, Cc, ho, wo, s12[0], s12[1], dg, db, False)
            held(dg.cpu(), want["dgamma"], SUMS_RTOL, f"{tag} train dgamma")
            held(db.cpu(), want["dbeta"], SUMS_RTOL, f"{tag} train dbeta")
            if elem == SP:
                s3, dg3, db3 = nans(3, G, Cc), nans(Cc), nans(Cc)
                ops.bn_relu_maxpool_bwd_reduce_split(gpd, am, yd, mean, invstd, scale, shift, G, N, H, W, Cc, ho, wo, s3[0], s3[1], dg3, db3, False, s3[2])
                same(s3[:2], s12, f"{tag} train split sums == fp32 sums")
                same(dg3, dg, f"{tag} train split dgamma == fp32")
                assert bool((s3[2] <= 4 * gpd.abs().amax(dim=(1, 2, 3)) * 1.0001).all())
                dy_f = nans(G, N, H, W, Cc)
                ops.bn_relu_maxpool_bwd_apply(gpd, am, yd, mean, invstd, gd, scale, shift, s12[0], s12[1], G, N, H, W, Cc, ho, wo, dy_f)
                dy = sp_nans(G, N, H, W, Cc)
                ops.bn_relu_maxpool_bwd_apply_split(gpd, am, yd, mean, invstd, gd, scale, shift, s3[0], s3[1], G, N, H, W, Cc, ho, wo, dy, s3[2])
                got = ops.merge_sp(dy)
                e = float((got - dy_f).abs().max()) / max(float(dy_f.abs().max()), 1e-30)
                print(f"BN-FORMS {tag} train dy vs the fp32 kernel: max error {e:.3e} of the maximum (bar 2^-22)")
                assert e <= 2.0 ** -22
                held(got.cpu(), dy_want, SUMS_RTOL, f"{tag} train dy")
            else:
                dy = nans(G, N, H, W, Cc, dtype=st_f32)
                ops.bn_relu_maxpool_bwd_apply(gpd, am, yd, mean, invstd, gd, scale, shift, s12[0], s12[1], G, N, H, W, Cc, ho, wo, dy)
                held(dy.float().cpu(), dy_want, OUT_RTOL if elem == BF16 else SUMS_RTOL, f"{tag} train dy")


@pytest.mark.parametrize("case", list(STEM_CASES), ids=lambda c: "g%d_n%d_%dx%d_c%d_cus%d" % c)
def test_stem_tail_reduce_counts_every_window_exactly_once(case):
    """Pooled gradient 1, the ReLU open everywhere (scale 0, shift 1), integer y and mean, invstd = 1: s1 EQUALS the number of
    pooling windows, s2 the integer sum of (y at the window's argmax - mean), in fp32, bf16 and the split form; the eval-mode
    pass leaves dy = gamma x the number of windows each pixel won."""
    from rot_mvgaze_amd import ops
    G, N, H, W, Cc, cus = case
    ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    gen = torch.Generator().manual_seed(H * W + Cc)
    y = torch.randint(-8, 9, (G, N, H, W, Cc), generator=gen).float()
    mean = torch.randint(-3, 4, (G, Cc), generator=gen).float()
    d = lambda t: t.to(dev())
    tag = "exact stem g%d_n%d_%dx%d_c%d_cus%d" % case
    one_gc, zero_gc = torch.ones(G, Cc), torch.zeros(G, Cc)
    with cus_left(cus), poisoned_workspaces():
        # the argmax of y itself (scale 1, shift 100: the ReLU changes nothing)
        am = torch.full((G, N, ho, wo, Cc), 0xFF, dtype=torch.uint8, device=dev())
        ops.bn_relu_maxpool_fwd(d(y), d(one_gc), d(one_gc * 100), nans(G, N, ho, wo, Cc), am, G, N, H, W, Cc, ho, wo)
        win, flat = _winner_values(y, am.cpu(), H, W)
        s2_want = (win.double() - mean.double()[:, None, None, None]).sum((1, 2, 3))
        n_win = float(N * ho * wo)
        for elem in (FP32, BF16, SP):
            guard_stem(elem, case, True)
            yd, gp = store(y, elem), store(torch.ones(G, N, ho, wo, Cc), elem)
            s, dg, db = nans(3, G, Cc), nans(Cc), nans(Cc)
            args = (gp, am, yd, d(mean), d(one_gc), d(zero_gc), d(one_gc), G, N, H, W, Cc, ho, wo, s[0], s[1], dg, db, False)
            if elem == SP:
                ops.bn_relu_maxpool_bwd_reduce_split(*args, s[2])
                same(s[2].cpu(), 4 * one_gc, f"{tag} sp mx == 4 x the largest window gradient")
            else:
                ops.bn_relu_maxpool_bwd_reduce(*args)
            same(s[0].cpu(), torch.full((G, Cc), n_win), f"{tag} {ELEM_NAMES[elem]} s1 == windows")
            same(s[1].cpu(), s2_want.float(), f"{tag} {ELEM_NAMES[elem]} s2")
            same(db.cpu(), torch.full((Cc,), G * n_win), f"{tag} {ELEM_NAMES[elem]} dbeta")
        guard_stem(FP32, case, False)
        rm = mean[0].contiguous()
        dy, dg, db = nans(G, N, H, W, Cc), nans(Cc), nans(Cc)
        ops.bn_relu_maxpool_eval_bwd(d(torch.ones(G, N, ho, wo, Cc)), am, d(y), d(zero_gc), d(one_gc), d(torch.full((Cc,), 2.0)), d(rm),
                                     d(torch.ones(Cc)), 0.0, G, N, H, W, Cc, ho, wo, dy, dg, db, False)
        won = torch.zeros(G, N, H * W * Cc).scatter_add_(2, flat.reshape(G, N, -1), torch.ones(G, N, ho * wo * Cc)).reshape(G, N, H, W, Cc)
        same(dy.cpu(), 2 * won, f"{tag} eval dy == gamma x windows won")
        same(db.cpu(), torch.full((Cc,), G * n_win), f"{tag} eval dbeta")
        same(dg.cpu(), (win.double() - rm.double()).sum((0, 1, 2, 3)).float(), f"{tag} eval dgamma")


def test_every_form_in_the_table_was_run():
    """Runs last in this file: what the guards saw is exactly FORMS (a case the planners moved elsewhere failed its own guard;
    a form nobody runs any more fails here)."""
    assert _seen == FORMS, f"not run: {sorted(FORMS - _seen)}; not in the table: {sorted(_seen - FORMS)}"
