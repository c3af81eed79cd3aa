"""Case tables and host arithmetic behind tests/test_bf16_forms_{cpu,gpu}.py, written from the descriptor and the documented
launch rules of csrc/conv_bf16.hip - not from the library.

The launch rule restated (launch_igemm_bf16): tiles are 128 rows x bn columns with bn = 128 when the GEMM has >= 128 columns,
else 64, K-steps of 64.  Forward: one class over every tap, K per tap = cin, columns = cout.  Backward-data: the classes of
igemm_forms_ref.class_table (stride 2: one per parity with a tap), K per tap = cout, columns = cin; the fused BatchNorm reduce
keeps the parity classes without a tap as epilogue-only classes of 0 K-steps.  The uniform-tap loader ("fasta") needs, in
every class, 1 .. 32 taps (0 allowed under the fused reduce) and K-per-tap a multiple of 64.  Kernel: the LDS-DMA kernel iff
fasta ("dma"), else the register-staged kernel ("reg"); the fp32-operand Linears ("mixed") always run the register-staged
kernel, fasta choosing its loader.  The fused reduce needs fasta.  K order: tap-major (64-channel block, tap) when a class
has more than one tap and K-per-tap is a multiple of 64.

Weight gradient (wgrad_bf16_impl): bm = 128 when cout >= 128 else 64, bn = 128 when r*s*cin >= 128 else 64; bf16 operands
step the pixel coordinates incrementally when ho*wo >= 128, fp32 operands (the mixed Linears) decode every step."""
import functools

import torch
import torch.nn.functional as F

from igemm_forms_ref import class_table, out_hw

BM, BK = 128, 64
DMA, REG = "dma", "reg"
E_RTOL = 2e-5                      # the project's fp32-accumulation bar (test_kernels_gpu.RTOL)


# ---------------------------------------------------------------- the launch rule, restated
def kept_class_table(case):
    """class_table(case, True) with the parity classes that have no tap kept (the fused BatchNorm reduce): longest K first,
    equal lengths in (py, px) order."""
    G, N, h, w, cin, cout, k, st, pad = case
    cls = []
    for py in range(st):
        for px in range(st):
            sub_h, sub_w = len(range(py, h, st)), len(range(px, w, st))
            nr = len([r for r in range(k) if (py + pad - r) % st == 0])
            ns = len([s for s in range(k) if (px + pad - s) % st == 0])
            if sub_h > 0 and sub_w > 0:
                cls.append((N * sub_h * sub_w, nr * ns, cout))
    return sorted(cls, key=lambda c: -c[1] * c[2])


def gemm_plan(case, dgrad, bnreduce=False):
    """(kernel, bn, fasta, tiles per class, K-steps per class) of a forward / backward-data launch on bf16 operands."""
    G, N, h, w, cin, cout, k, st, pad = case
    ncols, kc = (cin, cout) if dgrad else (cout, cin)
    bn = 128 if ncols >= 128 else 64
    tab = kept_class_table(case) if bnreduce else class_table(case, dgrad)
    fasta = all((1 <= taps or bnreduce) and taps <= 32 and kc % BK == 0 for _, taps, _ in tab)
    tiles = [G * -(-rows // BM) * -(-ncols // bn) for rows, _, _ in tab]
    kt = [-(-taps * kc // BK) if taps else (0 if bnreduce else 1) for _, taps, _ in tab]
    return (DMA if fasta else REG), bn, fasta, tiles, kt


def linear_case(rows, fin, fout):
    return (1, rows, 1, 1, fin, fout, 1, 1, 0)


def wgrad_tile(case, f32in=False):
    G, N, h, w, cin, cout, k, st, pad = case
    ho, wo = out_hw(case)
    return (128 if cout >= 128 else 64, 128 if k * k * cin >= 128 else 64, (not f32in) and ho * wo >= 128)


# ---------------------------------------------------------------- cases: (G, N, h, w, cin, cout, k, stride, pad)
# (case, forward form or None = not run, backward-data form or None); a form is (kernel, column tile)
GEMM_CASES = [
    ((1, 2, 9, 9, 64, 128, 3, 1, 1), (DMA, 128), (DMA, 64)),     # 162 rows: the last tile holds 34, its second wave row none
    ((2, 3, 7, 9, 128, 64, 1, 1, 0), (DMA, 64), (DMA, 128)),     # two groups; backward-data is ONE K-step
    ((1, 2, 8, 8, 64, 192, 1, 1, 0), (DMA, 128), (DMA, 64)),     # forward: ragged second column tile; backward: K of 3 steps
    ((1, 2, 8, 8, 192, 64, 1, 1, 0), None, (DMA, 128)),          # backward: ragged second column tile
    ((1, 2, 9, 9, 32, 128, 3, 1, 1), (REG, 128), None),          # two taps per K-step, ragged K tail (K = 288)
    ((1, 3, 9, 9, 32, 32, 3, 1, 1), (REG, 64), (REG, 64)),
    ((1, 2, 12, 12, 8, 64, 7, 2, 3), (REG, 64), (DMA, 64)),      # stem: channels 3..7 zero, K = 392; backward: 8 columns, 16/12/12/9 taps
    ((1, 1, 10, 10, 64, 64, 7, 2, 3), (REG, 64), (DMA, 64)),     # 49 taps of 64 channels: register-staged, tap-major K order
    ((1, 1, 10, 10, 128, 64, 7, 2, 3), (REG, 64), None),         # ... with two 64-channel blocks: the tap-major order differs from the plain one
    ((1, 2, 7, 7, 64, 64, 5, 1, 2), (DMA, 64), (DMA, 64)),       # 25 taps both ways
    ((1, 2, 9, 9, 128, 64, 3, 1, 1), None, (DMA, 128)),          # 9 taps
    ((2, 2, 9, 7, 64, 64, 3, 2, 1), None, (DMA, 64)),            # four ragged parity classes, 4/2/2/1 taps
    ((1, 2, 9, 9, 64, 64, 1, 2, 0), None, (DMA, 64)),            # three classes without a tap: the fill kernel
    ((1, 2, 9, 9, 128, 32, 3, 1, 1), None, (REG, 128)),
    ((1, 2, 9, 7, 128, 32, 3, 2, 1), None, (REG, 128)),          # ... with parity classes
]
# the inference epilogue over the four forward forms
AFFINE_CASES = [((1, 2, 9, 9, 64, 128, 3, 1, 1), (DMA, 128)), ((2, 3, 7, 9, 128, 64, 1, 1, 0), (DMA, 64)),
                ((1, 2, 9, 9, 32, 128, 3, 1, 1), (REG, 128)), ((1, 3, 9, 9, 32, 32, 3, 1, 1), (REG, 64))]
# mixed Linears (rows, fin, fout): (forward (fasta, bn), backward-data (fasta, bn))
LINEAR_CASES = [
    ((70, 64, 128), (True, 128), (True, 64)),
    ((70, 128, 64), (True, 64), (True, 128)),
    ((70, 72, 136), (False, 128), (False, 64)),                  # ragged K, ragged column tiles
    ((130, 136, 72), (False, 64), (False, 128)),                 # ... and a last row tile of 2 rows
]
# weight gradient on bf16 operands: (case, (bm, bn, incremental))
WGRAD_CASES = [
    ((1, 2, 12, 12, 128, 128, 1, 1, 0), (128, 128, True)),
    ((1, 5, 5, 5, 128, 128, 1, 1, 0), (128, 128, False)),
    ((1, 2, 12, 12, 16, 64, 3, 1, 1), (64, 128, True)),          # 144 columns
    ((1, 3, 5, 5, 32, 32, 3, 1, 1), (64, 128, False)),           # 32 of 64 rows, 288 columns
    ((1, 2, 12, 12, 64, 128, 1, 1, 0), (128, 64, True)),
    ((1, 3, 4, 4, 32, 192, 1, 1, 0), (128, 64, False)),          # ragged rows, 32 of 64 columns
    ((1, 2, 16, 8, 64, 64, 1, 1, 0), (64, 64, True)),            # exactly 128 pixels per image, wo = 8
    ((1, 4, 2, 2, 64, 96, 1, 1, 0), (64, 64, False)),            # 16 pixels: less than one K-step
    ((1, 2, 25, 23, 64, 64, 3, 2, 1), (64, 128, True)),          # stride 2, odd sizes
    ((1, 1, 2, 72, 64, 64, 1, 1, 0), (64, 64, True)),            # wo > 64
    ((2, 1, 12, 12, 8, 64, 7, 2, 3), (64, 128, False)),          # two groups
]
# the deferred path (slabs now, one batched sum): (case, splits) - the 1-, 4- and 16-lane sums
WGRAD_DEFER_CASES = [((1, 2, 12, 12, 128, 128, 1, 1, 0), 3), ((1, 2, 12, 12, 16, 64, 3, 1, 1), 9), ((1, 2, 25, 23, 64, 64, 3, 2, 1), 33)]
# weight gradient of the mixed Linears (rows, fin, fout): (bm, bn); always per-step decode
MIXED_WGRAD_CASES = [((70, 64, 128), (128, 64)), ((70, 128, 64), (64, 128)), ((70, 72, 136), (128, 64)), ((130, 136, 72), (64, 128)),
                     ((70, 128, 128), (128, 128)), ((70, 64, 64), (64, 64))]
# fused BatchNorm reduce (G, N, h, cin, cout, k, stride, pad) on h x h maps: column tile
REDUCE_CASES = [((1, 3, 9, 192, 128, 1, 1, 0), 128),             # ragged column tile
                ((2, 2, 9, 64, 64, 3, 2, 1), 64),
                ((1, 2, 9, 64, 64, 1, 2, 0), 64)]                # epilogue-only classes


def reduce_case(rc):
    G, N, h, cin, cout, k, st, pad = rc
    return (G, N, h, h, cin, cout, k, st, pad)


def wgrad_split_counts(case):
    """One split, three (the second and third start mid-image), and more splits than 64-pixel chunks (trailing empty ones)."""
    G, N, h, w, cin, cout, k, st, pad = case
    ho, wo = out_hw(case)
    return (1, 3, -(-G * N * ho * wo // 64) + 3)


# what must have run: the form-union test of the GPU file holds the recorded guards to this set
FORMS = (
    {(d, kern, bn) for d in ("fwd", "bwd") for kern in (DMA, REG) for bn in (128, 64)}                       # training: 8
    | {(d, fasta, bn) for d in ("lin_fwd", "lin_bwd") for fasta in (True, False) for bn in (128, 64)}       # mixed: 8
    | {("affine", kern, bn) for kern in (DMA, REG) for bn in (128, 64)}                                       # affine: 4
    | {("bnreduce", DMA, bn) for bn in (128, 64)}                                                             # fused reduce: 2
    | {("wgrad", bm, bn, incr) for bm in (128, 64) for bn in (128, 64) for incr in (True, False)}             # bf16 operands: 8
    | {("wgrad_mixed", bm, bn, False) for bm in (128, 64) for bn in (128, 64)}                                # fp32 operands: 4
)
assert len(FORMS) == 34


def table_forms():
    """The forms the tables above name."""
    out = set()
    for case, fwd, bwd in GEMM_CASES:
        out |= ({("fwd",) + fwd} if fwd else set()) | ({("bwd",) + bwd} if bwd else set())
    out |= {("affine",) + f for _, f in AFFINE_CASES}
    for _, fwd, bwd in LINEAR_CASES:
        out |= {("lin_fwd",) + fwd, ("lin_bwd",) + bwd}
    out |= {("bnreduce", DMA, bn) for _, bn in REDUCE_CASES}
    out |= {("wgrad",) + t for _, t in WGRAD_CASES} | {("wgrad_mixed",) + t + (False,) for _, t in MIXED_WGRAD_CASES}
    return out


# ---------------------------------------------------------------- the bar of a bf16 output
def bf16_bound(ref, magnitude):
    """Per-element bound of a bf16-stored result against float64 `ref`: 2^-8 |ref| (round to nearest at 8 significand bits) +
    1.004 E (the rounding of a value that is off by E moves with it), E = 2e-5 * M the fp32-accumulation bar, M = `magnitude`
    = the largest summed magnitude, over the elements, of the terms that enter an element before the rounding."""
    return ref.abs() * 2.0 ** -8 + 1.004 * E_RTOL * float(magnitude)


def bound_ratio(got, ref, magnitude):
    """max over the elements of |got - ref| / bound (<= 1 holds the bar); nothing is left out."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape
    bound = bf16_bound(ref, magnitude)
    if float(magnitude) == 0.0:
        return 0.0 if bool((got == ref).all()) else float("inf")
    return ((got - ref).abs() / bound).max().item()


# ---------------------------------------------------------------- problems: bf16-rounded operands and float64 references (CPU)
def q(t):
    return t.to(torch.bfloat16).float()


class GemmProblem:
    """x [G,N,h,w,cin], w [cout,k,k,cin] (fp32 master weights; wq its bf16 rounding), gy [G,N,ho,wo,cout], addend [G,N,h,w,cin] -
    all bf16-representable but w - and float64 y = conv(x, wq), dx = conv^T(gy, wq) in NHWC,
    dw = the weight gradient in KRSC.  A case with 8 input channels under
    a 7x7 filter is the stem: 3 real channels, image channels and weight channels 3..7 zero."""

    def __init__(self, case):
        G, N, h, w_, cin, cout, k, st, pad = case
        self.case = case
        ho, wo = out_hw(case)
        gen = torch.Generator().manual_seed(1000 + sum(c * (i + 1) for i, c in enumerate(case)))
        real = 3 if (cin == 8 and k == 7) else cin
        self.x = q(torch.randn(G, N, h, w_, cin, generator=gen))
        self.x[..., real:] = 0
        self.w = torch.randn(cout, k, k, cin, generator=gen) * (1.0 / (k * k * real) ** 0.5)
        self.w[..., real:] = 0
        self.cin_real = real
        self.wq = q(self.w)
        self.gy = q(torch.randn(G, N, ho, wo, cout, generator=gen))
        self.addend = q(torch.randn(G, N, h, w_, cin, generator=gen))
        self.y64, self.dx64, self.dw64 = self.conv(torch.float64)

    def conv(self, dtype):
        """(y, dx, dw) in `dtype` arithmetic on the rounded operands, NHWC / KRSC (dw summed over the groups)."""
        G, N, h, w_, cin, cout, k, st, pad = self.case
        ho, wo = out_hw(self.case)
        xr = self.x.to(dtype).reshape(G * N, h, w_, cin).permute(0, 3, 1, 2).requires_grad_(True)
        wr = self.wq.to(dtype).permute(0, 3, 1, 2).requires_grad_(True)
        y = F.conv2d(xr, wr, None, st, pad)
        y.backward(self.gy.to(dtype).reshape(G * N, ho, wo, cout).permute(0, 3, 1, 2))
        return (y.detach().permute(0, 2, 3, 1).reshape(G, N, ho, wo, cout).contiguous(),
                xr.grad.permute(0, 2, 3, 1).reshape(G, N, h, w_, cin).contiguous(), wr.grad.permute(0, 2, 3, 1).contiguous())


@functools.lru_cache(maxsize=None)
def gemm_problem(case):
    return GemmProblem(case)


def affine_operands(cout, shape):
    """Per-channel scale (both signs, zeros) and shift, and a bf16 residual of `shape`."""
    gen = torch.Generator().manual_seed(77 + cout)
    scale = torch.randn(cout, generator=gen)
    scale[::7] = 0.0
    assert float(scale.min()) < 0 < float(scale.max())
    return scale, torch.randn(cout, generator=gen) * 0.5, q(torch.randn(*shape, generator=gen))


class LinearProblem:
    """x [rows, fin], dy [rows, fout], mask / addend [rows, fin], bias [fout] in fp32 (the loaders round x and dy to bf16), w
    [fout, fin] fp32 master weights; float64 pre = q(x) wq^T, dx = q(dy) wq, dw = q(dy)^T q(x), db = column sums of the fp32 dy."""

    def __init__(self, rows, fin, fout):
        gen = torch.Generator().manual_seed(5000 + rows * 7 + fin * 3 + fout)
        self.x, self.dy = torch.randn(rows, fin, generator=gen), torch.randn(rows, fout, generator=gen)
        self.w = torch.randn(fout, fin, generator=gen) * fin ** -0.5
        self.bias = torch.randn(fout, generator=gen)
        self.mask, self.addend = torch.randn(rows, fin, generator=gen), torch.randn(rows, fin, generator=gen)
        xq, gq, wq = q(self.x).double(), q(self.dy).double(), q(self.w).double()
        self.pre64, self.dx64, self.dw64 = xq @ wq.T, gq @ wq, gq.T @ xq
        self.db64 = self.dy.double().sum(0)


@functools.lru_cache(maxsize=None)
def linear_problem(rows, fin, fout):
    return LinearProblem(rows, fin, fout)
