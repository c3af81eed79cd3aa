"""Host references and case tables behind tests/test_prep_forms_{cpu,gpu}.py: the operand producers (the sp split / merge
kernels, the batched weight prep, the stems' row-window builders) and the stems' conv forms.  numpy and torch on the CPU,
written from the comments of csrc/conv_split.hip, csrc/conv_bf16.hip and csrc/elem.h - not from the library.

The sp format (conv_split.hip's header): an fp32 value v as two fp16 pieces h1 = fp16(v), h2 = fp16(v - h1), round to nearest
even; channels in chunks of 8, the two pieces of a chunk adjacent: element (row, c, piece) at ushort offset
((row * C/8 + c/8) * 2 + piece) * 8 + c % 8."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

SP_ULP = 2.0 ** -23                 # |v - h1 - h2| <= 2^-23 |v| while h2 is a normal fp16 number
SP_FLOOR = 2.0 ** -25               # ... and an absolute 2^-25 (stored units) below: half the spacing of fp16's subnormals
RANGE_OVER_BITS = 0x477FF000        # 65520.0f: from here fp16 round-to-nearest-even gives inf (ops.split_f32_ranged)
SUBNORMAL_SHARE = 1e-3              # at most 0.1 % of a tensor may sit on the subnormal-piece exception


# ---------------------------------------------------------------- A. the sp format
def sp_pieces(v):
    """float32 [..., C] (C % 8 == 0) -> uint16 [..., C/8, 2, 8]: the stored pieces of v."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    assert v.shape[-1] % 8 == 0
    with np.errstate(over="ignore", invalid="ignore"):
        h1 = v.astype(np.float16)
        h2 = (v - h1.astype(np.float32)).astype(np.float16)
    lead = v.shape[:-1] + (v.shape[-1] // 8,)
    out = np.empty(lead + (2, 8), dtype=np.uint16)
    out[..., 0, :] = h1.view(np.uint16).reshape(lead + (8,))
    out[..., 1, :] = h2.view(np.uint16).reshape(lead + (8,))
    return out


def sp_merge(pieces, inv_scale=1.0):
    """uint16 [..., C/8, 2, 8] -> float32 [..., C]: (h1 + h2) * inv_scale in fp32 (mvg_merge_sp)."""
    h = np.ascontiguousarray(pieces).view(np.float16).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (h[..., 0, :] + h[..., 1, :]) * np.float32(inv_scale)
    return s.reshape(pieces.shape[:-3] + (pieces.shape[-3] * 8,))


def sp_scale_for(bound):
    """elem.h's sp_scale_for: the power of two that maps `bound` into [2^14, 2^15); 1 for a bound that is zero, negative, NaN
    or at least 3e38; the exponent clamped to +-100."""
    bound = float(np.float32(bound))
    if not (bound > 0.0) or not (bound < 3.0e38):
        return 1.0
    _, e = math.frexp(bound)                    # bound = m * 2^e, m in [0.5, 1)
    return math.ldexp(1.0, max(-100, min(100, 15 - e)))


def subnormal_piece(pieces):
    """Mask [..., C]: the reference's second piece is a nonzero fp16 subnormal (|h2| < 2^-14) - the one place where a device
    conversion that flushes instead of rounding may differ."""
    h2 = pieces[..., 1, :]
    m = ((h2 & 0x7C00) == 0) & ((h2 & 0x03FF) != 0)
    return m.reshape(pieces.shape[:-3] + (pieces.shape[-3] * 8,))


def sp_compare(got, stored):
    """The condition of the sp stores: `got` (uint16 [..., C/8, 2, 8], the device's pieces) against sp_pieces(stored), stored =
    the fp32 values handed to the split (v * scale).  Returns (wrong, excused, worst): elements whose pieces differ outside the
    exception; elements that differ under it; the largest |merged - stored| / (2^-23 |stored| + 2^-25) over the excused ones."""
    stored = np.ascontiguousarray(stored, dtype=np.float32)
    want = sp_pieces(stored)
    got = np.ascontiguousarray(got).reshape(want.shape)
    diff = (got != want).any(axis=-2).reshape(stored.shape)
    if not diff.any():
        return 0, 0, 0.0
    sub = subnormal_piece(want)
    wrong = int((diff & ~sub).sum())
    exc = diff & sub
    merged = sp_merge(got).astype(np.float64)[exc]
    s = stored.astype(np.float64)[exc]
    ratio = np.abs(merged - s) / (SP_ULP * np.abs(s) + SP_FLOOR)
    return wrong, int(exc.sum()), float(ratio.max()) if ratio.size else 0.0


def range_word(stored):
    """The integer maximum of the bits of |stored| (mvg_split_f32_ranged's record)."""
    b = np.ascontiguousarray(stored, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    return int(b.max()) if b.size else 0


SPLIT_SIZES = (8, 8 * 255, 8 * 257, 8 * (8192 * 256 + 3))          # one chunk; under / over one workgroup; past the 8192-block grid cap
# (name, magnitude of the values, scale): unscaled, a power-of-two scale, gradient-sized values at 2^28
SPLIT_SCALES = (("unit", 1.0, 1.0), ("pow2", 300.0, 2.0 ** -3), ("grad", 2.0 ** -20, 2.0 ** 28))


def split_values(n, mag, seed=0):
    """n fp32 values of magnitude `mag` over five decades, both signs, with the format's corner values in front."""
    g = np.random.default_rng(1234 + seed + n % 1000)
    v = (g.standard_normal(n) * mag * 10.0 ** g.uniform(-4.0, 0.5, n)).astype(np.float32)
    head = np.array([0.0, -0.0, 1.0, -1.0, 2.0 ** -10, 1e-3, -7.0, 0.333], dtype=np.float32) * np.float32(mag)
    v[:8] = head
    return v


# ---------------------------------------------------------------- B. the batched weight prep
# (name, cout, rs, cin, cin_pad, transposed copy?, magnitude)
MODE1_RECORDS = [
    ("3x3_64to128", 128, 9, 64, 64, True, 1.0),
    ("1x1_96to160", 160, 1, 96, 96, True, 1e-3),
    ("1x1_256to320", 320, 1, 256, 256, True, 300.0),           # 20 tiles: more than 16 workgroups, fewer than 64
    ("1x1_64to64", 64, 1, 64, 64, True, 0.08),                 # one tile
    ("1x1_128to64_no_wt", 64, 1, 128, 128, False, 7.0),        # a null transposed pointer
    ("stem_64x7x1x32", 64, 7, 32, 32, False, 0.08),
    ("zeros_3x3_32to32", 32, 9, 32, 32, True, 0.0),
]
MODE0_RECORDS = [
    ("1x1_256to320", 320, 1, 256, 256, True, 300.0),
    ("1x1_256to320_no_wt", 320, 1, 256, 256, False, 1e-3),
    ("3x3_64to128", 128, 9, 64, 64, True, 1.0),
    ("7x7_3to64_pad8", 64, 49, 3, 8, False, 0.08),
    ("stem_fold_128x7x1x64", 128, 7, 64, 64, False, 0.08),
    ("1x1_96to160", 160, 1, 96, 96, True, 7.0),
]
BLOCKS_PER_ITEM = (0, 16, 256)


def mode1_branch(rec):
    """weights_prep_batch_kernel, mode 1: how the transposed copy is made (the KRSC copy is the same loop for all)."""
    _, cout, rs, cin, cin_pad, wt, _ = rec
    if not wt:
        return "none"
    return "tiled" if (rs == 1 and cin % 64 == 0 and cout % 64 == 0) else "gather"


def mode0_branch(rec):
    _, cout, rs, cin, cin_pad, wt, _ = rec
    return "linear" if (rs == 1 and cin == cin_pad and cin % 64 == 0 and cout % 64 == 0) else "element"


def tiles(rec):
    _, cout, rs, cin, cin_pad, wt, _ = rec
    return (cout // 64) * (cin // 64)


def stem_taps_rowwindow(w):
    """w [cout, 7, 7, 3] -> w' [cout, 7, 8, 4] with w'[o][r][j][c] = w[o][r][j - 1][c], zero for j = 0 and c = 3."""
    w8 = torch.zeros(w.shape[0], 7, 8, 4, dtype=w.dtype)
    w8[:, :, 1:, :3] = w
    return w8


def stem_taps_folded(w):
    """w [cout, 7, 7, 3] -> w_fold [2 cout, 7, 16, 4] with w_fold[par * cout + o][r][j][c] = w[o][r][j - 1 - 2 par][c]."""
    cout = w.shape[0]
    w16 = torch.zeros(2 * cout, 7, 16, 4, dtype=w.dtype)
    w16[:cout, :, 1:8, :3] = w
    w16[cout:, :, 3:10, :3] = w
    return w16


def unfold_dw(dw16):
    cout = dw16.shape[0] // 2
    return dw16[:cout, :, 1:8, :3] + dw16[cout:, :, 3:10, :3]


@functools.lru_cache(maxsize=None)
def record_weights(mode, idx):
    """The fp32 source [cout, rs, cin] of a record (the stems' records in their tap layouts, zero taps included)."""
    rec = (MODE1_RECORDS if mode == 1 else MODE0_RECORDS)[idx]
    name, cout, rs, cin, cin_pad, wt, mag = rec
    gen = torch.Generator().manual_seed(100 * mode + idx)
    if name.startswith("stem_64"):
        w = stem_taps_rowwindow(torch.randn(64, 7, 7, 3, generator=gen) * mag).reshape(64, 7, 32)
    elif name.startswith("stem_fold"):
        w = stem_taps_folded(torch.randn(64, 7, 7, 3, generator=gen) * mag).reshape(128, 7, 64)
    elif mag == 0.0:
        w = torch.zeros(cout, rs, cin)
    else:
        w = torch.randn(cout, rs, cin, generator=gen) * mag
    return w.contiguous()


def mode1_expected(w):
    """(stat0 bits, stat1, scale, KRSC pieces' stored values [cout, rs*cin], CRSK's [cin, rs*cout]) of an fp32 source [cout, rs, cin]."""
    a = w.numpy()
    mx = np.float32(np.abs(a).max()) if a.size else np.float32(0)
    scale = sp_scale_for(mx)
    stored = a * np.float32(scale)                                  # a power of two: exact
    cout, rs, cin = a.shape
    return (int(mx.view(np.uint32)), np.float32(1.0 / scale), scale, stored.reshape(cout, rs * cin),
            np.ascontiguousarray(stored.transpose(2, 1, 0)).reshape(cin, rs * cout))


def mode0_expected(w, cin_pad):
    """(KRSC [cout, rs, cin_pad], CRSK [cin_pad, rs, cout]) in bf16 of an fp32 source [cout, rs, cin]; channels cin.. zero."""
    cout, rs, cin = w.shape
    wp = torch.zeros(cout, rs, cin_pad)
    wp[..., :cin] = w
    wk = wp.to(torch.bfloat16)
    return wk, wk.permute(2, 1, 0).contiguous()


# ---------------------------------------------------------------- C. the row-window builders
def rowwindow_split_ref(x_nhwc3):
    """numpy [images, H, W, 3] fp32 -> [images, H, W/2, 8, 4]: window ox, slot j = image column 2 ox - 4 + j, zero outside the
    image, channel 3 zero."""
    n, h, w, _ = x_nhwc3.shape
    wo = w // 2
    pad = np.zeros((n, h, w + 8, 4), dtype=np.float32)
    pad[:, :, 4:4 + w, :3] = x_nhwc3
    out = np.empty((n, h, wo, 8, 4), dtype=np.float32)
    for j in range(8):
        out[:, :, :, j] = pad[:, :, j:j + 2 * wo:2][:, :, :wo]      # padded column 2 ox + j = image column 2 ox - 4 + j
    return out


def rowwindow_bf16_ref(x_nhwc3):
    """numpy [images, H, W, 3] fp32 -> [images, H, W/4, 16, 4]: window m = image columns 4 m - 4 .. 4 m + 11."""
    n, h, w, _ = x_nhwc3.shape
    wm = w // 4
    pad = np.zeros((n, h, w + 16, 4), dtype=np.float32)
    pad[:, :, 4:4 + w, :3] = x_nhwc3
    out = np.empty((n, h, wm, 16, 4), dtype=np.float32)
    for j in range(16):
        out[:, :, :, j] = pad[:, :, j:j + 4 * wm:4][:, :, :wm]
    return out


# images, H, W.  The small ones of the two older stem tests, H = 1, windows that touch both borders, and one past 16384 x 256 threads
ROWWINDOW_SPLIT_SIZES = [(6, 32, 32), (4, 23, 40), (5, 7, 6), (3, 1, 10), (3, 5, 2), (33, 256, 256)]
ROWWINDOW_BF16_SIZES = [(8, 32, 32), (4, 24, 64), (24, 17, 32), (3, 1, 12), (3, 5, 4), (33, 256, 256)]


def image(n, h, w, seed=0):
    g = np.random.default_rng(77 + seed + n + 3 * h + 7 * w)
    return g.standard_normal((n, 3, h, w)).astype(np.float32)


# ---------------------------------------------------------------- D. the stems' conv forms
# the split stem: (G, N, H, W, cout); forward form (bm, bn, stages) per CU setting ("all CUs", "8 CUs"); weight-gradient form
SPLIT_STEM_CASES = [
    ((2, 2, 23, 40, 64), ((128, 64, 1), (128, 64, 1)), (64, 128, True)),       # odd H; 480 rows per group: last row tile 96
    ((1, 5, 7, 6, 64), ((128, 64, 1), (128, 64, 1)), (64, 128, False)),        # ho * wo = 12: per-step pixel decode
    ((1, 21, 113, 112, 64), ((256, 64, 1), (256, 64, 1)), (64, 128, True)),    # 67032 rows: 256-row tiles, the last one 216 rows
    ((1, 3, 63, 64, 128), ((128, 128, 2), (128, 128, 1)), (128, 128, True)),   # 24 tiles of 7 K-steps: pipelined / single-stage
    ((1, 2, 9, 8, 32), ((128, 64, 1), (128, 64, 1)), (64, 128, False)),        # a half-empty column tile
    ((1, 3, 16, 16, 96), ((128, 64, 1), (128, 64, 1)), (64, 128, True)),       # ragged second column tile (64 + 32), ragged row tile of dw
]
SPLIT_STEM_BIG = (1, 21, 113, 112, 64)                                         # forward only (the issue's 256 x 64 case)
SPLIT_STEM_FORMS = ({("split_fwd", 128, 64, 1), ("split_fwd", 256, 64, 1), ("split_fwd", 128, 128, 2), ("split_fwd", 128, 128, 1)}
                    | {("split_wgrad", 64, 128, True), ("split_wgrad", 64, 128, False), ("split_wgrad", 128, 128, True)})
# the bf16 folded stem: (G, N, H, W, cout); forward form (kernel, bn); weight-gradient form.  n * ho * (wo / 2) % 64 == 0
BF16_STEM_CASES = [
    ((2, 2, 24, 64, 64), ("dma", 128), (128, 128, True)),        # 192 folded rows per image
    ((1, 4, 16, 16, 64), ("dma", 128), (128, 128, False)),       # 32 per image; 128 folded rows
    ((1, 8, 17, 32, 32), ("dma", 64), (64, 128, False)),         # odd H; 576 folded rows: the last tile's second wave row is empty
    ((1, 2, 32, 32, 32), ("dma", 64), (64, 128, True)),          # exactly 128 per image
]
BF16_STEM_FORMS = ({("bf16_fwd", "dma", 128), ("bf16_fwd", "dma", 64)}
                   | {("bf16_wgrad", bm, 128, incr) for bm in (128, 64) for incr in (True, False)})
FORMS = SPLIT_STEM_FORMS | BF16_STEM_FORMS


def stem_out(H, W):
    return (H - 1) // 2 + 1, W // 2


def table_forms():
    out = set()
    for _, fwd, wg in SPLIT_STEM_CASES:
        out |= {("split_fwd",) + f for f in fwd} | {("split_wgrad",) + wg}
    for _, fwd, wg in BF16_STEM_CASES:
        out |= {("bf16_fwd",) + fwd, ("bf16_wgrad",) + wg}
    return out


def split_stem_plan(case, cus):
    """The launch rule of the split stem restated (split_plan / split_conv_stages / wgrad_split_tile on the rewritten descriptor:
    a 7 x 1 filter over 32 channels, cout GEMM columns): ((bm, bn, stages), (wgrad bm, bn, incremental)) with `cus` compute CUs."""
    G, N, H, W, cout = case
    ho, wo = stem_out(H, W)
    rows = N * ho * wo
    bn = 128 if cout >= 128 else 64
    bm = 256 if (cout < 128 and rows >= 65536) else 128
    ntiles = G * -(-rows // bm) * -(-cout // bn)
    pipelined = ntiles <= 2 * cus or (ntiles <= 4 * cus and 7 >= 48)
    stages = 2 if (pipelined and bn == 128 and bm == 128) else 1
    return (bm, bn, stages), (128 if cout >= 128 else 64, 128, ho * wo >= 32)


def bf16_stem_plan(case):
    G, N, H, W, cout = case
    ho, wo = stem_out(H, W)
    return ("dma", 128 if 2 * cout >= 128 else 64), (128 if 2 * cout >= 128 else 64, 128, ho * (wo // 2) >= 128)


def wgrad_split_counts(pixels, kstep, planned):
    """1, 2, the planner's own counts, and more slabs than K-steps (the trailing ones are empty)."""
    out = []
    for s in (1, 2) + tuple(planned) + (-(-pixels // kstep) + 3,):
        if s not in out:
            out.append(s)
    return out


class SplitStemProblem:
    """x [G,N,H,W,4] (channel 3 zero), w [cout,7,7,3], gy [G,N,ho,wo,cout] gradient-sized, and float64 y = conv2d(x, w, stride 2,
    pad 3) on the 3-channel image, dw [cout,7,7,3] by autograd (not for the big case, which is forward only)."""

    def __init__(self, case, backward=True):
        G, N, H, W, cout = case
        self.case = case
        ho, wo = stem_out(H, W)
        gen = torch.Generator().manual_seed(G * 1000 + H + W + cout)
        self.x = torch.randn(G, N, H, W, 4, generator=gen)
        self.x[..., 3] = 0
        self.w = torch.randn(cout, 7, 7, 3, generator=gen) * 0.08
        self.gy = torch.randn(G, N, ho, wo, cout, generator=gen) * 3e-4
        xr = self.x[..., :3].double().reshape(G * N, H, W, 3).permute(0, 3, 1, 2)
        wr = self.w.double().permute(0, 3, 1, 2).requires_grad_(backward)
        yr = F.conv2d(xr, wr, None, 2, 3)
        self.dw_ref = None
        if backward:
            yr.backward(self.gy.double().reshape(G * N, ho, wo, cout).permute(0, 3, 1, 2))
            self.dw_ref = wr.grad.permute(0, 2, 3, 1).contiguous()
        self.y_ref = yr.detach().permute(0, 2, 3, 1).reshape(G, N, ho, wo, cout).contiguous()


@functools.lru_cache(maxsize=2)
def split_stem_problem(case):
    return SplitStemProblem(case, backward=case != SPLIT_STEM_BIG)


class Bf16StemProblem:
    """bf16-representable x [G*N,3,H,W], w [cout,3,7,7], gy; float64 y [G,N,ho,wo,cout], dw [cout,7,7,3] on them, and M = the
    largest conv(|x|, |w|) (the magnitude of the per-element bar)."""

    def __init__(self, case):
        G, N, H, W, cout = case
        self.case = case
        ho, wo = stem_out(H, W)
        gen = torch.Generator().manual_seed(5 + G * 1000 + H + W + cout)
        q = lambda t: t.to(torch.bfloat16).float()
        self.x = q(torch.randn(G * N, 3, H, W, generator=gen))
        self.w = q(torch.randn(cout, 3, 7, 7, generator=gen) * (1.0 / 147 ** 0.5))
        self.gy = q(torch.randn(G, N, ho, wo, cout, generator=gen))
        wr = self.w.double().requires_grad_(True)
        yr = F.conv2d(self.x.double(), wr, None, 2, 3)
        yr.backward(self.gy.double().reshape(G * N, ho, wo, cout).permute(0, 3, 1, 2))
        self.y_ref = yr.detach().reshape(G, N, cout, ho, wo).permute(0, 1, 3, 4, 2).contiguous()
        self.dw_ref = wr.grad.permute(0, 2, 3, 1).contiguous()
        self.magnitude = float(F.conv2d(self.x.double().abs(), self.w.double().abs(), None, 2, 3).max())


@functools.lru_cache(maxsize=None)
def bf16_stem_problem(case):
    return Bf16StemProblem(case)


def partial_stats(block):
    """float64 [G, rows, C] -> (sum [G, C], centred sum of squares [G, C]) of one statistics partial's rows."""
    return block.sum(1), ((block - block.mean(1, keepdim=True)) ** 2).sum(1)
