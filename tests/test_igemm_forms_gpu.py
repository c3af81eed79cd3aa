"""Every launch form of the fp32-MFMA conv kernels (csrc/conv_igemm.hip) at kernel level, on small shapes.

Which instantiation of igemm_kernel a shape runs, and whether as one tile per workgroup or as a persistent stream-K grid with
igemm_fixup_kernel behind it, is decided on the host (choose_tile_multi, plan_streamk) from the CUs the planners may use.
ops.set_reserved_cus() moves the plan instead of the shape: with 8 - 16 CUs left, shapes of a few tiles run stream-K.  Every
case FIRST asserts through the host-only plan query (mvg_conv_plan_query / mvg_conv_wgrad_tile: answered by the code the
launches plan with) which instantiation and launch form it is about to run, and - for stream-K - that the registered scratch
holds the pieces (with less the launch would quietly take the plain form) and that the cuts of the unit space contain the
structures of igemm_forms_ref.streamk_structures the case is here for.  A later change of the cost model that moves a case fails
the guard instead of losing the coverage.  FORMS below is the table of what must have run; the last test asserts the union of
the guards' answers equals it.

Not reachable by a descriptor validate() accepts (left in the library, listed here): igemm_kernel<128, 128, 32, .., DGRAD = true>
(both loaders: tile_bk() steps backward-data by 16) and the plain forward <128, 128, 16> (tile_bk() steps that tile by 32; only the
rotate + concat loader of mvg_fuser_fprop has a 16-deep 128x128 forward instantiation, which the fuser test runs).  The
128x32 tile has a general-loader instantiation only.

Before every stream-K launch the stream's registered workspace is overwritten with 0xFF bytes (NaNs as floats): a fix-up that
read a slab slot this launch did not write would show in the output instead of finding the previous launch's values.  Each
stream-K launch runs twice, re-poisoned in between, and the two results must be torch.equal: the fix-up sums a tile's pieces in
workgroup order.  Stream-K against one-tile-per-workgroup results are NOT bit-equal (the K cuts differ); each is held to the bar.

Bars (the project's, not fitted here): float64 F.conv2d / autograd on the same fp32 inputs; test_kernels_gpu.close() with its
RTOL = 2e-5 (max error relative to max |reference|), K <= 4608 as in the cases that bar already holds for.  Every comparison
prints its relative L2 error as `IGEMM-FORMS <case> <form>: ...` before it asserts.

Measured on an MI355X (profiles/igemm_forms_errors.txt), relative L2 against float64, smallest .. largest over the cases (the
bar above is test_kernels_gpu.py's and was not refitted to these):
  forward                    stream-K 1.7e-07 .. 7.3e-07   one tile per workgroup 6.0e-08 .. 8.4e-07
  ... affine epilogue        stream-K 1.7e-07 .. 6.8e-07   one tile per workgroup 6.5e-08 .. 8.0e-07
  backward-data              stream-K 1.9e-07 .. 7.1e-07   one tile per workgroup 2.6e-08 .. 1.2e-06
  backward-weight            3.7e-08 .. 3.8e-07 over every tile, 1 / 3 / more splits than pixel chunks, fresh write and accumulate
  fuser forward              stream-K 5.5e-07              split-K 2.3e-07
On that device the planners see 2 / 5 resident workgroups per CU of the forward 128x128 / 128x64 kernels and 3 / 5 of the
backward-data ones; the persistent grids in igemm_forms_ref.STREAMK_CASES are those times the CUs left.
"""
import contextlib
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from igemm_forms_ref import (BWD, FWD, PLAIN_CASES, PLAIN_CUS, STREAMK_CASES, WGRAD_CASES, WGRAD_SPLITS_CASE, class_counts,
                             streamk_structures)
from test_kernels_gpu import RTOL, close, dev

pytestmark = pytest.mark.gpu

NAN = float("nan")

# (direction, bm, bn, bk, uniform-tap loader, stream-K): every instantiation launch_igemm can pick for an accepted descriptor,
# one tile per workgroup; the 128-row tiles with >= 64 columns also as stream-K
FORMS = {
    (FWD, 128, 128, 32, True, False), (FWD, 128, 128, 32, False, False), (FWD, 128, 64, 16, True, False),
    (FWD, 128, 64, 16, False, False), (FWD, 64, 64, 16, True, False), (FWD, 64, 64, 16, False, False),
    (FWD, 128, 32, 16, False, False),
    (BWD, 128, 128, 16, True, False), (BWD, 128, 128, 16, False, False), (BWD, 128, 64, 16, True, False),
    (BWD, 128, 64, 16, False, False), (BWD, 64, 64, 16, True, False), (BWD, 64, 64, 16, False, False),
    (BWD, 128, 32, 16, False, False),
    (FWD, 128, 128, 32, True, True), (FWD, 128, 64, 16, True, True), (BWD, 128, 128, 16, True, True),
    (BWD, 128, 64, 16, True, True),
}
_seen_forms = set()
_seen_structures = {FWD: set(), BWD: set()}


def rel_l2(got, ref):
    return ((got.double() - ref.double()).norm() / (ref.double().norm() + 1e-300)).item()


def held(got, ref, what):
    """Print the relative L2 error, then hold `got` to the family's bar."""
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values (an unwritten output or a stale scratch slot)"
    print(f"IGEMM-FORMS {what}: rel-L2 {rel_l2(got, ref):.3e}")
    close(got, ref, RTOL, what)


@contextlib.contextmanager
def cus_left(n):
    """Leave n CUs to the planners (0: all of them)."""
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import lib
    total = lib().mvg_device_cus()
    assert total >= 64, "the form guards are written for a device with many more than 16 CUs"
    try:
        ops.set_reserved_cus(total - n if n else 0)
        yield
    finally:
        ops.set_reserved_cus(0)


def poison_scratch():
    """0xFF over the current stream's registered workspace (registering it first, as the first launch would)."""
    from rot_mvgaze_amd import ops
    handle = ops._s(True)
    ws = ops._workspaces[(torch.cuda.current_device(), handle)]
    ws.fill_(0xFF)
    return ws.numel()


def desc(case):
    from rot_mvgaze_amd._lib import ConvDesc
    G, N, h, w_, cin, cout, k, st, pad = case
    return ConvDesc(G, N, h, w_, cin, cout, k, k, st, pad, (h + 2 * pad - k) // st + 1, (w_ + 2 * pad - k) // st + 1)


def cid(case):
    return "g%d_n%d_%dx%d_%dto%d_k%d_s%d" % tuple(case[:8])


def guard(direction, case, kind, tile, fasta, streamk, structures=None, grid=None):
    """Assert what the launch of `case` is about to run, from the library's own plan; record the form."""
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import lib
    pl = ops.conv_plan_query(desc(case), kind)
    got = (pl["bm"], pl["bn"], pl["bk"], pl["fasta"], pl["streamk_grid"] > 0)
    assert got == tuple(tile) + (fasta, streamk), f"{cid(case)}: the plan moved this case to {got} (grid {pl['streamk_grid']})"
    assert pl["splitk"] == 1
    tiles, kt = class_counts(case, direction == BWD, pl["bm"], pl["bn"], pl["bk"])
    assert (pl["cls_tiles"], pl["cls_kt"]) == (tiles, kt), f"{cid(case)}: classes {pl['cls_tiles']} x {pl['cls_kt']}"
    if streamk:
        assert 0 < pl["scratch_floats"] * 4 <= lib().mvg_scratch_bytes() == poison_scratch(), \
            "the registered scratch does not hold the stream-K pieces: the launch would take the plain form"
        assert grid is None or pl["streamk_grid"] == grid, f"{cid(case)}: {pl['streamk_grid']} persistent workgroups"
        found = streamk_structures(pl["cls_tiles"], pl["cls_kt"], pl["streamk_grid"])
        assert structures is None or found == set(structures), f"{cid(case)}: structures {sorted(found)}"
        _seen_structures[direction] |= found
    else:
        assert pl["scratch_floats"] == 0
    _seen_forms.add((direction,) + got)
    return pl


class Problem:
    """Inputs of one conv and its float64 reference on the device: y, dx (from autograd) for a unit-sized dy."""

    def __init__(self, case, backward):
        G, N, h, w_, cin, cout, k, st, pad = case
        torch.manual_seed(sum(case))
        self.d = d = desc(case)
        self.x = torch.relu(torch.randn(G, N, h, w_, cin, device=dev()))
        self.w = torch.randn(cout, k, k, cin, device=dev()) * (1.0 / (k * k * cin) ** 0.5)
        self.gy = torch.randn(G, N, d.ho, d.wo, cout, device=dev())
        xr = self.x.double().view(G * N, h, w_, cin).permute(0, 3, 1, 2).requires_grad_(backward)
        wr = self.w.double().permute(0, 3, 1, 2)
        yr = F.conv2d(xr, wr, None, st, pad)
        self.y_ref = yr.detach().permute(0, 2, 3, 1).reshape(G, N, d.ho, d.wo, cout)
        if backward:
            yr.backward(self.gy.double().view(G * N, d.ho, d.wo, cout).permute(0, 3, 1, 2))
            self.dx_ref = xr.grad.permute(0, 2, 3, 1).reshape(self.x.shape)


def twice(launch, shape, streamk, what):
    """Run `launch(out)` into a NaN-filled output; under stream-K twice, the scratch poisoned before each, bit-equal results."""
    outs = []
    for _ in range(2 if streamk else 1):
        if streamk:
            poison_scratch()
        out = torch.full(shape, NAN, device=dev())
        launch(out)
        outs.append(out)
    if streamk:
        assert torch.equal(outs[0], outs[1]), f"{what}: two stream-K launches of the same inputs differ"
    return outs[0]


def check_stats(pb, y, stats, P, rpp, what):
    """The BatchNorm statistics partials against y's own rows (sums; squares centred on the partial's mean), then bn_finalize's
    mean and invstd against float64."""
    from rot_mvgaze_amd import ops
    d = pb.d
    G, cout, rows = d.groups, d.cout, d.n * d.ho * d.wo
    covered = (rows + rpp - 1) // rpp
    yg = y.view(G, rows, cout).double()
    for p in range(covered):
        blk = yg[:, p * rpp:min((p + 1) * rpp, rows)]
        torch.testing.assert_close(stats[:, p, 0].double(), blk.sum(1), rtol=1e-4, atol=1e-4 * float(blk.abs().sum(1).max()))
        q = ((blk - blk.mean(1, keepdim=True)) ** 2).sum(1)
        torch.testing.assert_close(stats[:, p, 1].double(), q, rtol=1e-3, atol=1e-5 * float(q.max()) + 1e-12)
    gamma, beta = torch.rand(cout, device=dev()) + 0.5, torch.randn(cout, device=dev()) * 0.1
    rm, rv = torch.zeros(cout, device=dev()), torch.ones(cout, device=dev())
    mean, invstd, scale, shift = (torch.full((G, cout), NAN, device=dev()) for _ in range(4))
    ops.bn_finalize(stats, G, P, rpp, rows, cout, gamma, beta, rm, rv, 0.1, 1e-5, mean, invstd, scale, shift)
    ref = pb.y_ref.reshape(G, rows, cout)
    close(mean, ref.mean(1), 1e-5, what + " bn mean")
    close(invstd, 1.0 / torch.sqrt(ref.var(1, unbiased=False) + 1e-5), 1e-5, what + " bn invstd")


def run_forward(pb, case, tile, fasta, streamk, form, structures=None, grid=None, epilogues=True):
    """mvg_conv_fprop plain / bias + ReLU / with statistics partials, mvg_conv_fprop_affine with and without residual + ReLU."""
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import PLAN_FPROP, PLAN_FPROP_STATS
    d, name = pb.d, cid(case)
    shape = pb.y_ref.shape
    guard(FWD, case, PLAN_FPROP, tile, fasta, streamk, structures, grid)
    y = twice(lambda o: ops.conv_fprop(d, pb.x, pb.w, o, None, False, None), shape, streamk, f"{name} {form} fprop")
    held(y, pb.y_ref, f"{name} {form} fprop")
    if not epilogues:
        return
    bias = torch.randn(d.cout, device=dev())
    yb = twice(lambda o: ops.conv_fprop(d, pb.x, pb.w, o, bias, True, None), shape, streamk, f"{name} {form} fprop+bias+relu")
    held(yb, torch.relu(pb.y_ref + bias.double()), f"{name} {form} fprop+bias+relu")
    guard(FWD, case, PLAN_FPROP_STATS, tile, fasta, streamk, structures, grid)
    P, rpp = ops.conv_stats_partials(d)                     # plans with the CU count too: asked under the same reserve
    stats = torch.full((d.groups, P, 2, d.cout), NAN, device=dev())
    ys = twice(lambda o: ops.conv_fprop(d, pb.x, pb.w, o, None, False, stats), shape, streamk, f"{name} {form} fprop+stats")
    held(ys, pb.y_ref, f"{name} {form} fprop+stats")
    check_stats(pb, ys, stats, P, rpp, f"{name} {form}")
    scale, shift = torch.rand(d.cout, device=dev()) + 0.5, torch.randn(d.cout, device=dev()) * 0.3
    res = torch.randn(shape, device=dev())
    for r, relu in ((res, True), (None, False), (res, False), (None, True)):
        ref = pb.y_ref * scale.double() + shift.double()
        if r is not None:
            ref = ref + r.double()
        if relu:
            ref = torch.relu(ref)
        what = f"{name} {form} fprop_affine{'+residual' if r is not None else ''}{'+relu' if relu else ''}"
        out = twice(lambda o: ops.conv_fprop_affine(d, pb.x, pb.w, o, scale, shift, r, relu), shape, streamk, what)
        held(out, ref, what)


def run_backward(pb, case, tile, fasta, streamk, form, structures=None, grid=None):
    """mvg_conv_dgrad plain, and with mask + addend aliasing dx."""
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import PLAN_DGRAD
    d, name = pb.d, cid(case)
    guard(BWD, case, PLAN_DGRAD, tile, fasta, streamk, structures, grid)
    dx = twice(lambda o: ops.conv_dgrad(d, pb.gy, pb.w, o), pb.x.shape, streamk, f"{name} {form} dgrad")
    held(dx, pb.dx_ref, f"{name} {form} dgrad")
    mask, add = torch.randn(pb.x.shape, device=dev()), torch.randn(pb.x.shape, device=dev())

    def in_place(o):
        o.copy_(add)
        ops.conv_dgrad(d, pb.gy, pb.w, o, mask, o)
    dx2 = twice(in_place, pb.x.shape, streamk, f"{name} {form} dgrad+mask+addend")
    held(dx2, pb.dx_ref * (mask > 0) + add.double(), f"{name} {form} dgrad+mask+addend in place")


@pytest.mark.parametrize("direction,case,cus,tile,grid,structures", STREAMK_CASES, ids=[c[0] + "_" + cid(c[1]) for c in STREAMK_CASES])
def test_streamk_and_the_same_shape_with_every_cu(direction, case, cus, tile, grid, structures):
    """The case under stream-K (guarded: instantiation, persistent grid, the structures of its cuts, scratch) with every epilogue
    of its direction; then the same shape with no CU reserved, one tile per workgroup."""
    pb = Problem(case, direction == BWD)
    run = run_forward if direction == FWD else run_backward
    with cus_left(cus):
        run(pb, case, tile, True, True, "%dx%dx%d stream-K" % tile, structures, grid)
    with cus_left(0):
        run(pb, case, (64, 64, 16), True, False, "64x64x16 plain")


@pytest.mark.parametrize("direction,case,form", PLAIN_CASES, ids=[c[0] + "_" + cid(c[1]) for c in PLAIN_CASES])
def test_every_instantiation_one_tile_per_workgroup(direction, case, form):
    pb = Problem(case, direction == BWD)
    run = run_forward if direction == FWD else run_backward
    with cus_left(PLAIN_CUS):
        run(pb, case, form[:3], form[3], False, "%dx%dx%d%s plain" % (form[:3] + (" uniform-tap" if form[3] else " general",)))


def wgrad_reference(case):
    G, N, h, w_, cin, cout, k, st, pad = case
    torch.manual_seed(sum(case) + 1)
    d = desc(case)
    x = torch.relu(torch.randn(G, N, h, w_, cin, device=dev()))
    gy = torch.randn(G, N, d.ho, d.wo, cout, device=dev())
    wr = torch.zeros(cout, cin, k, k, dtype=torch.float64, device=dev(), requires_grad=True)
    yr = F.conv2d(x.double().view(G * N, h, w_, cin).permute(0, 3, 1, 2), wr, None, st, pad)
    yr.backward(gy.double().view(G * N, d.ho, d.wo, cout).permute(0, 3, 1, 2))
    return d, x, gy, wr.grad.permute(0, 2, 3, 1).contiguous()


def wgrad_with_splits(d, x, gy, dw, splits, accumulate):
    """mvg_conv_wgrad with a split count of the caller's choice (ops.conv_wgrad takes the planner's)."""
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import check, lib
    ws = torch.full((splits * dw.numel(),), NAN, device=dev()) if splits > 1 else None
    check(lib().mvg_conv_wgrad(C.byref(d), ops._p(x), ops._p(gy), ops._p(dw), ops._p(ws), splits, int(accumulate), ops._s()),
          "conv_wgrad")


@pytest.mark.parametrize("case,form", WGRAD_CASES, ids=[cid(c) for c, _ in WGRAD_CASES])
def test_wgrad_every_tile_and_pixel_addressing(case, form):
    """One case per (tile, incremental) pair of wgrad_tile(): one split, several, and more splits than 16-pixel chunks (the
    trailing splits are empty and must write zeros); fresh write and accumulate."""
    from rot_mvgaze_amd import ops
    d, x, gy, dw_ref = wgrad_reference(case)
    assert ops.conv_wgrad_tile(d) == form, "this shape no longer runs the tile form it is here for"
    pixels = d.groups * d.n * d.ho * d.wo
    chunks = (pixels + 15) // 16
    what = "%s wgrad %dx%d%s" % ((cid(case),) + form[:2] + (" incr" if form[2] else "",))
    for splits in (1, 3, chunks + 3):
        dw = torch.full(dw_ref.shape, NAN, device=dev())
        wgrad_with_splits(d, x, gy, dw, splits, False)
        held(dw, dw_ref, f"{what} {splits} splits")
        acc = torch.ones_like(dw)
        wgrad_with_splits(d, x, gy, acc, splits, True)
        held(acc, dw_ref + 1.0, f"{what} {splits} splits accumulate")


def test_wgrad_planned_splits_follow_the_cus():
    """mvg_conv_wgrad_splits plans with the CU count: 36 tiles get several splits on every CU and one on 8; both are right."""
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import lib
    d, x, gy, dw_ref = wgrad_reference(WGRAD_SPLITS_CASE)
    assert ops.conv_wgrad_tile(d) == (128, 128, True)
    n = []
    for cus in (0, 8):
        with cus_left(cus):
            n.append(lib().mvg_conv_wgrad_splits(C.byref(d)))
            dw = torch.full(dw_ref.shape, NAN, device=dev())
            ops.conv_wgrad(d, x, gy, dw, False)
            held(dw, dw_ref, f"{cid(WGRAD_SPLITS_CASE)} wgrad 128x128 incr {n[-1]} planned splits")
            ops.conv_wgrad(d, x, gy, dw, True)
            held(dw, 2 * dw_ref, f"{cid(WGRAD_SPLITS_CASE)} wgrad 128x128 incr {n[-1]} planned splits accumulate")
    assert n[0] > 1 and n[1] == 1, f"planned splits {n}"


def test_fuser_loader_under_streamk_and_splitk():
    """mvg_fuser_fprop (rows generated by the rotate + concat loader) as 9 tiles of 128x128 x 224 K-steps: stream-K on 8 CUs,
    split-K with every CU; both against rotcat_fwd + a float64 matmul."""
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import ConvDesc, PLAN_FUSER_FPROP, lib
    V, B, cf, nvec, fout = 2, 550, 2048, 512, 128
    D, rows, kin = 2, 2 * 550, 2048 + 3 * 512
    torch.manual_seed(5)
    img, feat = torch.randn(V, B, cf, device=dev()), torch.randn(V, B, 3, nvec, device=dev())
    rel = torch.randn(D, B, 3, 3, device=dev())
    w, bias = torch.randn(fout, kin, device=dev()) * kin ** -0.5, torch.randn(fout, device=dev())
    vi, vj = torch.tensor([0, 1], dtype=torch.int32, device=dev()), torch.tensor([1, 0], dtype=torch.int32, device=dev())
    X = torch.empty(rows, kin, device=dev())
    ops.rotcat_fwd(img, feat, rel, vi, vj, X, B, D, cf, nvec)
    ref = torch.relu(X.double() @ w.double().t() + bias.double())
    b_idx = torch.arange(B, dtype=torch.int32, device=dev())
    row_img, row_src = (vi[:, None] * B + b_idx[None]).reshape(-1).contiguous(), (vj[:, None] * B + b_idx[None]).reshape(-1).contiguous()
    d = ConvDesc.linear(rows, kin, fout)
    ws_floats = lib().mvg_linear_workspace_floats(rows, kin, fout)

    def launch(o):
        ops.fuser_fprop(img.reshape(V * B, cf), feat.reshape(V * B, 3 * nvec), rel, row_img, row_src, w, bias, True, o, rows, cf, nvec, fout)
    with cus_left(8):
        pl = ops.conv_plan_query(d, PLAN_FUSER_FPROP, ws_floats)
        assert (pl["bm"], pl["bn"], pl["bk"], pl["fasta"], pl["splitk"]) == (128, 128, 16, True, 1) and pl["streamk_grid"] > 0, pl
        assert (pl["cls_tiles"], pl["cls_kt"]) == ([9], [224])
        assert 0 < pl["scratch_floats"] * 4 <= lib().mvg_scratch_bytes() == poison_scratch()
        held(twice(launch, (rows, fout), True, "fuser_fprop stream-K"), ref, "fuser_fprop 128x128x16 rotate+concat stream-K")
    with cus_left(0):
        pl = ops.conv_plan_query(d, PLAN_FUSER_FPROP, ws_floats)
        assert pl["splitk"] > 1 and pl["streamk_grid"] == 0, pl
        held(twice(launch, (rows, fout), False, "fuser_fprop split-K"), ref,
             "fuser_fprop %dx%dx16 rotate+concat split-K x%d" % (pl["bm"], pl["bn"], pl["splitk"]))


def test_zz_every_form_and_structure_is_guarded():
    """The union of the plan's answers over the case lists - what the guards above assert case by case - is every instantiation
    and launch form of FORMS, and every stream-K structure in both directions ((g), (h) need several classes: backward-data
    only).  Whatever the tests of this file that ran before this one recorded is part of that union."""
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import PLAN_DGRAD, PLAN_FPROP
    forms, structures = set(), {FWD: set(), BWD: set()}
    runs = [(dr, case, cus) for dr, case, cus, _, _, _ in STREAMK_CASES] + [(dr, case, 0) for dr, case, _, _, _, _ in STREAMK_CASES] + \
           [(dr, case, PLAIN_CUS) for dr, case, _ in PLAIN_CASES]
    for dr, case, cus in runs:
        with cus_left(cus):
            pl = ops.conv_plan_query(desc(case), PLAN_DGRAD if dr == BWD else PLAN_FPROP)
        forms.add((dr, pl["bm"], pl["bn"], pl["bk"], pl["fasta"], pl["streamk_grid"] > 0))
        if pl["streamk_grid"] > 0:
            structures[dr] |= streamk_structures(pl["cls_tiles"], pl["cls_kt"], pl["streamk_grid"])
    assert forms == FORMS, f"missing {sorted(FORMS - forms)}, unexpected {sorted(forms - FORMS)}"
    assert _seen_forms <= FORMS, sorted(_seen_forms - FORMS)
    assert structures[FWD] == set("abcdef"), sorted(structures[FWD])
    assert structures[BWD] == set("abcdefgh"), sorted(structures[BWD])
    assert _seen_structures[FWD] <= structures[FWD] and _seen_structures[BWD] <= structures[BWD]
