"""Every launch form of the bf16 storage path's conv kernels (csrc/conv_bf16.hip, conv_bf16_gemm.inc, the bf16 and fp32-operand
forms of bf16_tile.h's epilogue) at kernel level, on small shapes.

Which kernel a shape runs - the LDS-DMA kernel or the register-staged one, at 128 or 64 columns, with which K order and how many
classes; which weight-gradient tile with which pixel addressing - is decided on the host.  Every case FIRST asserts through the
host-only plan query (mvg_conv_plan_query_bf16 / mvg_conv_wgrad_tile_bf16: answered by the code the launches plan with) which
form it is about to run and records it; the last test asserts that the union of the recorded forms equals bf16_forms_ref.FORMS
(written out there: 8 training, 8 mixed, 4 affine, 2 fused-reduce, 8 + 4 weight-gradient forms).  A later change of the launch
rule that moves a case fails its guard instead of losing the coverage.  The stem's folded forms are test_bf16_gpu.py's.

Every output and every slab workspace starts as NaN (an element the launch does not write shows), inside a larger allocation
with a sentinel margin on both sides that must be bit-unchanged afterwards (a store past either end shows).

References: float64 on the same bf16-rounded operands (F.conv2d / autograd, matrix products), bf16_forms_ref's problems.
Bars - none fitted to the kernels:
  bf16 outputs (y, dx, the affine output), per element, nothing left out: |got - ref| <= 2^-8 |ref| + 1.004 E, E = 2e-5 M
      (bf16_forms_ref.bf16_bound: round to nearest at 8 significand bits of a value within the project's fp32-accumulation bar E;
      M = the largest summed magnitude of the terms entering an element - |conv * scale| + |shift| + |residual|, or |conv| +
      |addend|; ReLU and masks are 1-Lipschitz or exact).  It implies test_bf16_gpu.close(.., OUT_RTOL); a store that truncates
      instead of rounding misses it on a large share of the elements (tests/test_bf16_forms_cpu.py), which OUT_RTOL accepts.
  fp32 outputs (dw, db, the mixed Linears' y / dx): test_bf16_gpu.close(.., 2e-5); db 1e-5.
  forward statistics, each 64-row partial on its own: its sum and its centred sum of squares close(.., 2e-4) against float64
      over those rows; a partial without rows exactly (0, 0).
  fused reduce: dx per element as above AND bit-equal, with the sums, to mvg_conv_dgrad_bf16 followed by the reduce pass; s1, s2,
      dgamma, dbeta also against float64 sums over the device's own stored dx at 2e-5 max(|want|, 1) sqrt(rows).
Every comparison prints its largest bound ratio (bf16 outputs) or relative L2 (fp32 outputs) as `BF16-FORMS <case> <form>: ...`
before it asserts; profiles/bf16_forms_errors.txt holds an MI355X's.

Measured on an MI355X (profiles/bf16_forms_errors.txt), smallest .. largest over the cases (the bars above were not fitted to these):
  bf16 outputs, largest bound ratio   forward 0.917 .. 0.979, backward-data 0.930 .. 0.982, affine 0.940 .. 0.968, fused reduce 0.946 .. 0.982
                                      (fp32 arithmetic rounded once, on the CPU: 0.956 .. 0.982, tests/test_bf16_forms_cpu.py)
  fp32 outputs, relative L2           mixed Linears 2.9e-08 .. 6.3e-08, weight gradients 2.0e-08 .. 9.4e-08, bias gradients 8.8e-08 .. 1.4e-07
  forward statistics per partial      1.3e-07 .. 4.0e-07 of the partial's largest sum / centred sum of squares

Two things the cases taught.  The tap-major K order is a permutation of the K-steps that the register-staged loader applies to
both operands from one index, so a loader that ignores it altogether computes the same sums: only a loader in which ONE operand
ignores it is wrong, and only where a tap spans more than one 64-channel block - the 49-tap case with 128 channels per tap is
here for that (at 64 channels per tap both orders are the same order).  And the separate reduce pass rejects 192 channels
(24 chunks of 8 do not divide 256), which the fused launch serves with a ragged column tile: there the two-launch reference
masks the stored gradient itself (test_bf16_forms_fused_reduce).

Not reachable through the C ABI, so not here: a bias gradient on the bf16-operand weight gradient (no entry point passes one)."""
import ctypes as C

import pytest
import torch

import rot_mvgaze_amd  # noqa: F401
import bf16_forms_ref as R
from test_bf16_gpu import close, dev

pytestmark = pytest.mark.gpu

NAN = float("nan")
MARGIN = 4096                        # sentinel elements on either side of an output
_seen = set()


def cid(case):
    return "x".join(map(str, case))


def rel_l2(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return ((got - ref).norm() / (ref.norm() + 1e-300)).item()


class Guarded:
    """An output tensor `.t` of `shape` inside a larger allocation: NaN (or `init`) inside, a bit pattern on both sides."""

    def __init__(self, shape, dtype=torch.float32, init=None):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.empty(n + 2 * MARGIN, dtype=dtype, device=dev())
        self.ints = self.buf.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)
        self.sentinel = 0x5A5A if dtype == torch.bfloat16 else 0x5A5A5A5A
        self.ints.fill_(self.sentinel)
        self.t = self.buf[MARGIN:MARGIN + n].view(shape)
        if init is None:
            self.t.fill_(NAN)
        else:
            self.t.copy_(init)

    def intact(self, what):
        ok = bool((self.ints[:MARGIN] == self.sentinel).all()) and bool((self.ints[-MARGIN:] == self.sentinel).all())
        assert ok, f"{what}: the launch wrote outside its output"
        return self.t


def held_bf16(out, ref, magnitude, what):
    """A bf16 output against float64, element by element (bf16_forms_ref.bf16_bound)."""
    got = out.intact(what) if isinstance(out, Guarded) else out
    assert got.dtype == torch.bfloat16
    assert bool(torch.isfinite(got.float()).all()), f"{what}: non-finite values (an element the launch did not write)"
    ratio = R.bound_ratio(got, ref, magnitude)
    print(f"BF16-FORMS {what}: largest bound ratio {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: an element is at {ratio:.3f} of its bound 2^-8 |ref| + 1.004 * 2e-5 * {float(magnitude):.3e}"


def held_f32(out, ref, what, rtol=2e-5):
    got = out.intact(what) if isinstance(out, Guarded) else out
    assert got.dtype == torch.float32
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values (an unwritten output, or an unwritten slab summed into it)"
    print(f"BF16-FORMS {what}: rel-L2 {rel_l2(got, ref):.3e}")
    close(got, ref, rtol, what)


def desc(case):
    from rot_mvgaze_amd._lib import ConvDesc
    return ConvDesc.make(*case)


def guard(tag, case, kind, form, bnreduce=False):
    """Assert what the launch of `case` is about to run, from the library's own plan; record the form."""
    from rot_mvgaze_amd import ops
    pl = ops.conv_plan_query_bf16(desc(case), kind)
    kernel, bn, fasta, tiles, kt = R.gemm_plan(case, tag in ("bwd", "bnreduce", "lin_bwd"), bnreduce)
    got = (pl["fasta"], pl["bn"]) if tag.startswith("lin_") else (pl["kernel"], pl["bn"])
    assert got == tuple(form), f"{cid(case)} {tag}: the plan moved this case to {got}"
    assert (pl["bm"], pl["bk"], pl["fasta"], pl["cls_tiles"], pl["cls_kt"]) == (128, 64, fasta, tiles, kt), f"{cid(case)} {tag}: {pl}"
    assert (pl["kernel"] == "mixed") == tag.startswith("lin_")
    _seen.add((tag,) + got)
    return "%s%d" % (pl["kernel"], pl["bn"])


def guard_wgrad(case, tile, f32in=False):
    from rot_mvgaze_amd import ops
    got = ops.conv_wgrad_tile_bf16(desc(case), f32in)
    assert got == tuple(tile), f"{cid(case)}: the weight gradient moved to {got}"
    _seen.add(("wgrad_mixed" if f32in else "wgrad",) + got)
    return "%dx%d%s" % (got[0], got[1], "incr" if got[2] else "decode")


def operands(p):
    """The problem's tensors on the device: x, gy, addend (bf16 NHWC), the bf16 weight copies (KRSC, CRSK) through the cast kernel."""
    from rot_mvgaze_amd import ops
    d = desc(p.case)
    wk, wt = ops.cast_weights_bf16(d, p.w[..., :p.cin_real].contiguous().to(dev()), p.cin_real, True)
    assert torch.equal(wk.float().cpu(), p.wq), "cast: the KRSC copy is the rounded master weight, padding channels zero"
    bf = lambda t: t.to(torch.bfloat16).to(dev())
    return d, bf(p.x), bf(p.gy), bf(p.addend), wk, wt


FWD_CASES = [(c, f) for c, f, _ in R.GEMM_CASES if f is not None]
BWD_CASES = [(c, b) for c, _, b in R.GEMM_CASES if b is not None]


@pytest.mark.parametrize("case,form", FWD_CASES, ids=[cid(c) for c, _ in FWD_CASES])
def test_bf16_forms_forward_and_statistics(case, form):
    from rot_mvgaze_amd import _lib, ops
    name = guard("fwd", case, _lib.PLAN_BF16_FPROP, form)
    p = R.gemm_problem(case)
    d, xd, _, _, wk, _ = operands(p)
    G, cout, rows = case[0], case[5], case[1] * d.ho * d.wo
    P, rpp = ops.conv_stats_partials(d, True)
    assert (P, rpp) == (2 * -(-rows // 128), 64)
    y, stats = Guarded((G, case[1], d.ho, d.wo, cout), torch.bfloat16), Guarded((G, P, 2, cout))
    ops.conv_fprop(d, xd, wk, y.t, None, False, stats.t)
    held_bf16(y, p.y64, p.y64.abs().max(), f"{cid(case)} fwd {name} y")
    st = stats.intact("stats").cpu().double()
    assert bool(torch.isfinite(st).all()), "a partial was not written"
    yg = p.y64.reshape(G, rows, cout)
    worst = [0.0, 0.0]
    for pi in range(P):
        part = yg[:, 64 * pi:64 * pi + 64]
        if part.shape[1] == 0:
            assert bool((st[:, pi] == 0).all()), f"partial {pi} holds no rows: it must be exactly (0, 0)"
            continue
        want = (part.sum(1), ((part - part.mean(1, keepdim=True)) ** 2).sum(1))
        for g in range(G):
            for k in range(2):
                err = (st[g, pi, k] - want[k][g]).abs().max().item() / (want[k][g].abs().max().item() + 1e-300)
                worst[k] = max(worst[k], err)
    print(f"BF16-FORMS {cid(case)} fwd {name} partials: sum {worst[0]:.3e} centred squares {worst[1]:.3e} (of the partial's largest)")
    assert max(worst) <= 2e-4, f"a partial's sum / centred sum of squares: {worst}"
    if 0 < rows % 128 <= 64:
        assert bool((st[:, P - 1] == 0).all()) and bool((st[:, P - 2, 0] != 0).any())         # the empty wave row's partial
    y2 = Guarded((G, case[1], d.ho, d.wo, cout), torch.bfloat16)
    ops.conv_fprop(d, xd, wk, y2.t, None, False, None)
    assert torch.equal(y2.intact("y without statistics"), y.t), "the statistics must not change y"


@pytest.mark.parametrize("case,form", BWD_CASES, ids=[cid(c) for c, _ in BWD_CASES])
def test_bf16_forms_backward_data(case, form):
    """Plain, + addend (another tensor), + mask and addend, and the in-place addend; a 1x1 stride-2 filter leaves three parity
    classes to the fill kernel (zeros, or the addend)."""
    from rot_mvgaze_amd import _lib, ops
    name = guard("bwd", case, _lib.PLAN_BF16_DGRAD, form)
    p = R.gemm_problem(case)
    d, _, gyd, addd, _, wt = operands(p)
    shape = tuple(p.dx64.shape)
    what = f"{cid(case)} bwd {name}"
    dx = Guarded(shape, torch.bfloat16)
    ops.conv_dgrad(d, gyd, wt, dx.t)
    held_bf16(dx, p.dx64, p.dx64.abs().max(), what + " dx")
    a64 = p.addend.double()
    mag = (p.dx64.abs() + a64.abs()).max()
    dxa = Guarded(shape, torch.bfloat16)
    ops.conv_dgrad(d, gyd, wt, dxa.t, None, addd)
    held_bf16(dxa, p.dx64 + a64, mag, what + " dx + addend")
    assert torch.equal(addd.cpu(), p.addend.to(torch.bfloat16)), "the addend was written"
    mask = torch.roll(p.addend, 1, dims=-2)                                        # bf16 values of both signs
    dxm = Guarded(shape, torch.bfloat16)
    ops.conv_dgrad(d, gyd, wt, dxm.t, mask.to(torch.bfloat16).to(dev()), addd)
    held_bf16(dxm, p.dx64 * (mask > 0) + a64, mag, what + " dx * mask + addend")
    dxi = Guarded(shape, torch.bfloat16, init=addd)
    ops.conv_dgrad(d, gyd, wt, dxi.t, None, dxi.t)
    assert torch.equal(dxi.intact(what + " in place"), dxa.t), "the in-place addend must give the same bits"


@pytest.mark.parametrize("case,form", R.AFFINE_CASES, ids=[cid(c) for c, _ in R.AFFINE_CASES])
def test_bf16_forms_affine_epilogue(case, form):
    from rot_mvgaze_amd import _lib, ops
    name = guard("affine", case, _lib.PLAN_BF16_AFFINE, form)
    p = R.gemm_problem(case)
    d, xd, _, _, wk, _ = operands(p)
    shape, cout = tuple(p.y64.shape), case[5]
    scale, shift, res = R.affine_operands(cout, shape)
    scale_d, shift_d, res_d = scale.to(dev()), shift.to(dev()), res.to(torch.bfloat16).to(dev())
    for with_res in (False, True):
        for relu in (False, True):
            out = Guarded(shape, torch.bfloat16)
            ops.conv_fprop_bf16_affine(d, xd, wk, out.t, scale_d, shift_d, res_d if with_res else None, relu)
            ref = p.y64 * scale.double() + shift.double()
            mag = (p.y64 * scale.double()).abs() + shift.double().abs()
            if with_res:
                ref, mag = ref + res.double(), mag + res.double().abs()
            held_bf16(out, torch.relu(ref) if relu else ref, mag.max(), f"{cid(case)} affine {name} residual={with_res} relu={relu}")
    assert torch.equal(res_d.cpu(), res.to(torch.bfloat16)), "the residual was written"
    plain, ident = Guarded(shape, torch.bfloat16), Guarded(shape, torch.bfloat16)
    ops.conv_fprop(d, xd, wk, plain.t, None, False, None)
    ops.conv_fprop_bf16_affine(d, xd, wk, ident.t, torch.ones(cout, device=dev()), torch.zeros(cout, device=dev()), None, False)
    assert torch.equal(ident.intact("identity affine"), plain.intact("plain")), "scale 1 / shift 0 must reproduce mvg_conv_fprop_bf16"


@pytest.mark.parametrize("lin,fwd,bwd", R.LINEAR_CASES, ids=[cid(c) for c, _, _ in R.LINEAR_CASES])
def test_bf16_forms_mixed_linears(lin, fwd, bwd):
    """mvg_linear_fprop_mixed over {bias, none} x {relu, none}; mvg_linear_dgrad_mixed over {mask + addend, addend, mask, neither}
    (neither, at whole column tiles: the two-quads-per-lane epilogue)."""
    from rot_mvgaze_amd import _lib, ops
    rows, fin, fout = lin
    case = R.linear_case(*lin)
    nf = guard("lin_fwd", case, _lib.PLAN_BF16_LINEAR_FPROP_MIXED, fwd)
    nb = guard("lin_bwd", case, _lib.PLAN_BF16_LINEAR_DGRAD_MIXED, bwd)
    p = R.linear_problem(*lin)
    wk, wt = ops.cast_weights_bf16(_lib.ConvDesc.linear(1, fin, fout), p.w.to(dev()), fin, True)
    xd, gd, bd, md, ad = (t.to(dev()) for t in (p.x, p.dy, p.bias, p.mask, p.addend))
    for bias in (True, False):
        for relu in (True, False):
            y = Guarded((rows, fout))
            ops.linear_fprop_mixed(xd, wk, bd if bias else None, relu, y.t, rows, fin, fout)
            ref = p.pre64 + (p.bias.double() if bias else 0.0)
            held_f32(y, torch.relu(ref) if relu else ref, f"{cid(lin)} lin_fwd {nf} fasta={fwd[0]} bias={bias} relu={relu}")
    for with_mask in (True, False):
        for with_add in (True, False):
            dx = Guarded((rows, fin))
            ops.linear_dgrad_mixed(gd, wt, md if with_mask else None, ad if with_add else None, dx.t, rows, fin, fout)
            ref = p.dx64 * (p.mask > 0) if with_mask else p.dx64
            held_f32(dx, ref + p.addend.double() if with_add else ref, f"{cid(lin)} lin_bwd {nb} fasta={bwd[0]} mask={with_mask} addend={with_add}")
    dxi = Guarded((rows, fin), init=ad)
    ops.linear_dgrad_mixed(gd, wt, None, dxi.t, dxi.t, rows, fin, fout)
    held_f32(dxi, p.dx64 + p.addend.double(), f"{cid(lin)} lin_bwd {nb} in-place addend")


@pytest.mark.parametrize("mask", ["bits", "affine", "none"])
@pytest.mark.parametrize("rc,bn", R.REDUCE_CASES, ids=[cid(c) for c, _ in R.REDUCE_CASES])
def test_bf16_forms_fused_reduce(rc, bn, mask):
    from rot_mvgaze_amd import _lib, ops
    case = R.reduce_case(rc)
    name = guard("bnreduce", case, _lib.PLAN_BF16_DGRAD_BNREDUCE, (R.DMA, bn), bnreduce=True)
    G, N, h, _, cin, cout, k, st, pad = case
    p = R.gemm_problem(case)
    d, _, gyd, addd, _, wt = operands(p)
    rows = N * h * h
    gen = torch.Generator().manual_seed(31 + sum(rc))
    y = R.q(torch.randn(G, rows, cin, generator=gen) * 1.5 + 0.3)
    mean, invstd = torch.randn(G, cin, generator=gen) * 0.1 + 0.3, torch.rand(G, cin, generator=gen) + 0.4
    scale, shift = torch.rand(G, cin, generator=gen) + 0.5, torch.randn(G, cin, generator=gen) * 0.3
    bits = torch.randint(0, 256, (G * rows * cin // 8,), dtype=torch.uint8, generator=gen)
    yd, meand, invstdd = y.to(torch.bfloat16).to(dev()), mean.to(dev()), invstd.to(dev())
    bitsd = bits.to(dev()) if mask == "bits" else None
    ra = (scale.to(dev()), shift.to(dev())) if mask == "affine" else None
    on = torch.ones(G, rows, cin, dtype=torch.bool)
    if mask == "bits":
        on = ((bits.view(-1, 1) >> torch.arange(8, dtype=torch.uint8)) & 1).bool().view(G, rows, cin)
    elif mask == "affine":
        on = y.double() * scale.double()[:, None] + shift.double()[:, None] > 0
    # two launches: backward-data, then the reduce pass over its stored result
    dx_ref = torch.empty(G, N, h, h, cin, dtype=torch.bfloat16, device=dev())
    ops.conv_dgrad(d, gyd, wt, dx_ref, None, addd)
    s_ref = [torch.empty(G, cin, device=dev()) for _ in range(2)]
    dg_ref, db_ref = torch.full((cin,), 0.5, device=dev()), torch.full((cin,), -0.25, device=dev())
    g2 = dx_ref.view(G, rows, cin)
    # the reduce pass serves widths whose 8-channel chunks divide 256 (or exceed it): 192 channels, which the fused launch takes
    # with a ragged column tile, it rejects - there its masked gradient is written here, an exact selection on the stored
    # values, and the sums are held to float64 alone
    pass_serves = 256 % (cin // 8) == 0 or cin // 8 > 256

    def reduce_pass():
        if mask == "bits":
            ops.bn_bwd_reduce_bits(g2, bitsd, yd, meand, invstdd, G, rows, cin, s_ref[0], s_ref[1], dg_ref, db_ref, True, dz_out=g2)
        else:
            ops.bn_bwd_reduce(g2, None, yd, meand, invstdd, G, rows, cin, s_ref[0], s_ref[1], dg_ref, db_ref, True, ra, dz_out=g2)

    if pass_serves:
        reduce_pass()
    else:
        with pytest.raises(RuntimeError, match="must divide 256"):
            reduce_pass()
        g2.copy_(torch.where(on.to(dev()), g2, torch.zeros_like(g2)))
    # fused
    dx = Guarded((G, N, h, h, cin), torch.bfloat16)
    s = [Guarded((G, cin)) for _ in range(2)]
    dg, db = Guarded((cin,), init=torch.full((cin,), 0.5)), Guarded((cin,), init=torch.full((cin,), -0.25))
    ops.conv_dgrad_bf16_bnreduce(d, gyd, wt, dx.t, addd, yd, bitsd, meand, invstdd, ra, s[0].t, s[1].t, dg.t, db.t, True)
    what = f"{cid(rc)} bnreduce {name} mask={mask}"
    a64 = p.addend.double()
    held_bf16(dx, (p.dx64 + a64) * on.view(G, N, h, h, cin), (p.dx64.abs() + a64.abs()).max(), what + " dx")
    assert torch.equal(dx.t, dx_ref), what + ": the masked gradient differs from backward-data followed by the reduce pass"
    dz = dx.t.float().cpu().double().view(G, rows, cin)
    want = [dz.sum(1), (dz * (y.double() - mean.double()[:, None]) * invstd.double()[:, None]).sum(1)]
    want += [0.5 + want[1].sum(0), -0.25 + want[0].sum(0)]
    for got, two, w64, nm in ((s[0], s_ref[0], want[0], "s1"), (s[1], s_ref[1], want[1], "s2"), (dg, dg_ref, want[2], "dgamma"),
                              (db, db_ref, want[3], "dbeta")):
        g = got.intact(nm).cpu().double()
        assert bool(torch.isfinite(g).all()), nm
        e2 = (g - two.cpu().double()).abs().max().item() if pass_serves else 0.0
        e64 = (g - w64).abs().max().item()
        tol = 2e-5 * max(w64.abs().max().item(), 1.0) * rows ** 0.5
        print(f"BF16-FORMS {what} {nm}: vs two launches {e2 if pass_serves else NAN:.3e}, vs float64 over the stored dx {e64:.3e} (bound {tol:.3e})")
        assert (not pass_serves or e2 <= 2e-5 * max(two.abs().max().item(), 1.0) * rows ** 0.5) and e64 <= tol, f"{nm}: {e2:.3e} {e64:.3e}"
    dxi = Guarded((G, N, h, h, cin), torch.bfloat16, init=addd)                     # in-place addend, no dgamma / dbeta
    s2 = [Guarded((G, cin)) for _ in range(2)]
    ops.conv_dgrad_bf16_bnreduce(d, gyd, wt, dxi.t, dxi.t, yd, bitsd, meand, invstdd, ra, s2[0].t, s2[1].t, None, None, False)
    assert torch.equal(dxi.intact("in place"), dx_ref) and torch.equal(s2[0].intact("s1"), s[0].t) and torch.equal(s2[1].intact("s2"), s[1].t)


def _wgrad_call(d, xd, gyd, dw, ws, splits, accumulate):
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import check, lib
    check(lib().mvg_conv_wgrad_bf16(C.byref(d), ops._p(xd), ops._p(gyd), ops._p(dw), ops._p(ws), splits, int(accumulate), ops._s()),
          "conv_wgrad_bf16")


@pytest.mark.parametrize("case,tile", R.WGRAD_CASES, ids=[cid(c) for c, _ in R.WGRAD_CASES])
def test_bf16_forms_weight_gradient_with_caller_chosen_splits(case, tile):
    """mvg_conv_wgrad_bf16 with 1 split, 3 (the later ones start mid-image) and more splits than 64-pixel chunks (the trailing
    ones are empty and must contribute zeros - their slabs start as NaN), fresh write and accumulate."""
    name = guard_wgrad(case, tile)
    p = R.gemm_problem(case)
    d, xd, gyd, _, _, _ = operands(p)
    n = p.dw64.numel()
    base = torch.randn(p.dw64.shape, generator=torch.Generator().manual_seed(3))
    for splits in R.wgrad_split_counts(case):
        for accumulate in (False, True):
            dw = Guarded(tuple(p.dw64.shape), init=base if accumulate else None)
            ws = Guarded((splits * n,)) if splits > 1 else None
            _wgrad_call(d, xd, gyd, dw.t, ws.t if ws else None, splits, accumulate)
            if ws:
                ws.intact("slabs")
            held_f32(dw, p.dw64 + base.double() if accumulate else p.dw64, f"{cid(case)} wgrad {name} splits={splits} accumulate={accumulate}")


@pytest.mark.parametrize("lin,tile", R.MIXED_WGRAD_CASES, ids=[cid(c) for c, _ in R.MIXED_WGRAD_CASES])
def test_bf16_forms_mixed_weight_and_bias_gradient(lin, tile):
    """mvg_linear_wgrad_mixed at the same three split counts: with more than one the bias slabs sit behind the weight slabs in a
    workspace of splits * (fout * fin + fout) floats and are summed by a reduce of their own."""
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import check, lib
    rows, fin, fout = lin
    case = R.linear_case(*lin)
    name = guard_wgrad(case, tile + (False,), f32in=True)
    p = R.linear_problem(*lin)
    xd, gd = p.x.to(dev()), p.dy.to(dev())
    gen = torch.Generator().manual_seed(4)
    bw, bb = torch.randn(fout, fin, generator=gen), torch.randn(fout, generator=gen)
    for splits in R.wgrad_split_counts(case):
        for accumulate in (False, True):
            dw, db = Guarded((fout, fin), init=bw if accumulate else None), Guarded((fout,), init=bb if accumulate else None)
            ws = Guarded((splits * (fout * fin + fout),)) if splits > 1 else None
            check(lib().mvg_linear_wgrad_mixed(ops._p(xd), ops._p(gd), ops._p(dw.t), ops._p(db.t), rows, fin, fout, ops._p(ws.t if ws else None),
                                               splits, int(accumulate), ops._s()), "linear_wgrad_mixed")
            if ws:
                ws.intact("slabs")
            what = f"{cid(lin)} wgrad_mixed {name} splits={splits} accumulate={accumulate}"
            held_f32(dw, p.dw64 + bw.double() if accumulate else p.dw64, what + " dw")
            held_f32(db, p.db64 + bb.double() if accumulate else p.db64, what + " db", 1e-5)


def test_bf16_forms_deferred_slab_sums():
    """What every bf16 training step runs: mvg_conv_wgrad_bf16_slabs per layer, then ONE mvg_wgrad_reduce_batch over the items - here
    with 3, 9 and 33 splits (1, 4 and 16 lanes per column), accumulate mixed.  Same slabs, same sum, same lanes as
    mvg_conv_wgrad_bf16 at that split count: equal bits."""
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import check, lib
    items, checks = [], []
    for i, (case, splits) in enumerate(R.WGRAD_DEFER_CASES):
        guard_wgrad(case, dict(R.WGRAD_CASES)[case])
        p = R.gemm_problem(case)
        d, xd, gyd, _, _, _ = operands(p)
        accumulate = i != 1
        base = torch.randn(p.dw64.shape, generator=torch.Generator().manual_seed(5 + i))
        direct, ws_d = Guarded(tuple(p.dw64.shape), init=base), Guarded((splits * p.dw64.numel(),))
        _wgrad_call(d, xd, gyd, direct.t, ws_d.t, splits, accumulate)
        ws, dw = Guarded((splits * p.dw64.numel(),)), Guarded(tuple(p.dw64.shape), init=base if accumulate else None)
        check(lib().mvg_conv_wgrad_bf16_slabs(C.byref(d), ops._p(xd), ops._p(gyd), ops._p(ws.t), splits, ops._s()), "conv_wgrad_bf16_slabs")
        assert torch.equal(ws.intact("slabs"), ws_d.intact("slabs")), "the deferred launch writes the slabs of the direct one"
        assert bool(torch.isfinite(ws.t).all()), "a slab element was not written"
        items.append((ws.t, dw.t, splits, accumulate))
        checks.append((case, splits, accumulate, dw, direct, p.dw64 + base.double() if accumulate else p.dw64))
    ops.wgrad_reduce_batch(items)
    for case, splits, accumulate, dw, direct, ref in checks:
        what = f"{cid(case)} wgrad deferred splits={splits} accumulate={accumulate}"
        held_f32(dw, ref, what)
        assert torch.equal(dw.t, direct.intact(what)), what + ": not the bits of mvg_conv_wgrad_bf16 at the same split count"


def test_bf16_forms_rejections():
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import lib
    case = R.WGRAD_CASES[0][0]
    p = R.gemm_problem(case)
    d, xd, gyd, addd, _, wt = operands(p)
    ws = Guarded((3 * p.dw64.numel(),))
    L = lib()
    assert L.mvg_conv_wgrad_bf16_slabs(C.byref(d), ops._p(xd), ops._p(gyd), ops._p(ws.t), 1, ops._s()) != 0         # one split: no slabs
    assert L.mvg_conv_wgrad_bf16_slabs(C.byref(d), ops._p(xd), ops._p(gyd), None, 3, ops._s()) != 0                 # no workspace
    assert L.mvg_conv_wgrad_bf16(C.byref(d), ops._p(xd), ops._p(gyd), ops._p(ws.t), None, 3, 0, ops._s()) != 0
    assert bool(torch.isnan(ws.intact("workspace")).all()), "a rejected call launched"
    # the fused reduce at 32 output channels per tap: rejected before anything is launched
    narrow = (1, 2, 9, 9, 64, 32, 1, 1, 0)
    pn = R.gemm_problem(narrow)
    dn, _, gyn, addn, _, wtn = operands(pn)
    dx = Guarded(tuple(pn.dx64.shape), torch.bfloat16)
    y = torch.zeros(1, 2 * 81, 64, dtype=torch.bfloat16, device=dev())
    one = torch.ones(1, 64, device=dev())
    s1, s2 = torch.empty(1, 64, device=dev()), torch.empty(1, 64, device=dev())
    with pytest.raises(RuntimeError, match="multiples of 64"):
        ops.conv_dgrad_bf16_bnreduce(dn, gyn, wtn, dx.t, addn, y, None, one, one, None, s1, s2, None, None, False)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx.intact("dx").float()).all()), "a rejected call launched"


def test_bf16_forms_union_of_guarded_forms():
    """Runs last: what the guards above recorded is the whole table."""
    assert _seen == R.FORMS, f"never run: {sorted(R.FORMS - _seen, key=str)}; not in the table: {sorted(_seen - R.FORMS, key=str)}"
