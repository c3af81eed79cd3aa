"""Case tables, inputs, float64 references and derived bars behind tests/test_fusion_split_forms_{cpu,gpu}.py: the fusion block's
Linears on the split kernels (mvg_linear_fprop_split / _dgrad_split / _wgrad_split) and the operand builders around them
(mvg_split_colsum, mvg_absmax_multi, mvg_fuse_build_split, mvg_fuse_unbuild).  numpy and torch on the CPU, written from the comments
of csrc/conv_split.hip, csrc/fusion.hip, csrc/bf16_tile.h and csrc/elem.h - not from the library.

The plan of a Linear launch (split_plan with lin): 128-row tiles; with C = the CUs the planners may use, 64-column tiles iff the GEMM
has fewer than 128 columns or 2 * ceil(rows / 128) * ceil(columns / 128) <= C; the two-stage K loop iff tiles <= 2 C, or tiles <= 4 C
and K-steps (of 32 inputs) >= 48.  Columns: fout forward, fin in backward-data.  ops.set_reserved_cus moves C instead of the shape:
the tables name, per case, the (bn, stages) of the three settings - every CU of a 256-CU device, 16 CUs, 8 CUs."""
import functools
import itertools

import numpy as np
import torch

from prep_forms_ref import SUBNORMAL_SHARE, sp_compare, sp_merge, sp_pieces, sp_scale_for  # noqa: F401  (re-exported to the tests)

U = 2.0 ** -24                       # fp32's unit roundoff
SETTING_CUS = (("all CUs", None), ("16 CUs", 16), ("8 CUs", 8))        # None: nothing reserved
DEVICE_CUS = 256                     # what the tables are written for (the planners assume it where there is no device)


def settings(cus):
    """(name, CUs to reserve) per setting on a device with `cus` CUs."""
    return tuple((name, 0 if keep is None else cus - keep) for name, keep in SETTING_CUS)


def linear_plan(rows, fin, fout, dgrad, cus):
    """split_plan(.., lin = true, ..) restated: (bn, stages) of a Linear launch with `cus` compute CUs."""
    ncols, k = (fin, fout) if dgrad else (fout, fin)
    mt = -(-rows // 128)
    bn = 128 if ncols >= 128 else 64
    if bn == 128 and 2 * mt * -(-ncols // 128) <= cus:
        bn = 64
    tiles = mt * -(-ncols // bn)
    pipelined = tiles <= 2 * cus or (tiles <= 4 * cus and -(-k // 32) >= 48)
    return bn, 2 if pipelined else 1


# (rows, fin, fout) forward; backward-data runs the mirrored Linear (rows, fout, fin): `fin` of the row in the column role, the same
# forms.  ((bn, stages) under all CUs, 16 CUs, 8 CUs), and what the case is here for
LINEAR_CASES = [
    ((300, 64, 800), ((64, 2), (128, 2), (128, 1)), "39 / 21 / 21 tiles: ragged seventh column tile of 32, ragged third row tile, 2 K-steps"),
    ((384, 64, 768), ((64, 2), (128, 2), (128, 1)), "the exact-fit twin: 18 tiles of 128 x 128"),
    ((1100, 96, 96), ((64, 2), (64, 2), (64, 1)), "18 tiles of 128 x 64, ragged second column tile, 3 K-steps"),
    ((300, 1536, 800), ((64, 2), (128, 2), (128, 2)), "48 K-steps: at 8 CUs 21 tiles are pipelined by the long-K rule"),
    ((200, 32, 160), ((64, 2), (64, 2), (64, 2)), "one K-step: the pipelined loop runs its prologue only"),
    ((200, 64, 160), ((64, 2), (64, 2), (64, 2)), "two K-steps (even)"),
    ((200, 96, 160), ((64, 2), (64, 2), (64, 2)), "three K-steps (odd)"),
    ((300, 32, 800), ((64, 2), (128, 2), (128, 1)), "one K-step on 128-column tiles, both K loops"),
    ((300, 96, 800), ((64, 2), (128, 2), (128, 1)), "three K-steps on 128-column tiles, both K loops"),
    ((1, 64, 160), ((64, 2), (64, 2), (64, 2)), "one row"),
    ((127, 64, 160), ((64, 2), (64, 2), (64, 2)), "one row short of a tile"),
    ((129, 64, 160), ((64, 2), (64, 2), (64, 2)), "one row into the second tile"),
    ((129, 64, 672), ((64, 2), (128, 2), (128, 2)), "one row into the second tile, 128-column tiles with a ragged sixth of 32"),
]
LONG_K_BOUNDARY = ((300, 1536, 800), (300, 1504, 800))      # 48 / 47 K-steps at 21 tiles on 8 CUs: two stages / one
TILES = ((128, 256), (128, 192), (128, 128), (128, 64), (64, 192), (64, 128), (64, 64))
FORMS = ({("linear", bn, stages, dgrad) for bn in (128, 64) for stages in (1, 2) for dgrad in (False, True)}
         | {("wgrad",) + t for t in TILES})

# (rows, fin, fout), tile (fout rows x fin columns of dw), whether the slab count must differ between all CUs and 8 CUs
WGRAD_CASES = [
    ((200, 256, 128), (128, 256), False),
    ((1100, 192, 160), (128, 192), False),      # ragged second row tile (160 = 128 + 32); 69 K-steps of 16 rows, the last of 12
    ((1, 128, 128), (128, 128), False),         # one row in a 16-row K-step
    ((1100, 160, 128), (128, 128), False),      # ragged second column tile
    ((200, 96, 128), (128, 64), False),         # ragged second column tile; 13 K-steps, the last of 8
    ((1100, 192, 64), (64, 192), False),
    ((200, 256, 96), (64, 128), False),         # ragged second row tile (96 = 64 + 32)
    ((1, 64, 32), (64, 64), False),             # half-empty tile
    ((1100, 768, 256), (128, 256), True),       # 6 tiles: four slabs on every CU, two on 8
    ((1100, 960, 256), (128, 192), True),       # 10 tiles: four slabs / two
]


def wgrad_tile(rows, fin, fout):
    """wgrad_split_tile on ConvDesc.linear restated: (bm, bn)."""
    bm = 128 if fout >= 128 else 64
    bn = 128 if fin >= 128 else 64
    if bm == 128 and fin >= 256 and fin % 256 == 0:
        bn = 256
    elif fin % 192 == 0:
        bn = 192
    return bm, bn


def table_forms():
    out = set()
    for (rows, fin, fout), forms, _ in LINEAR_CASES:
        out |= {("linear", bn, st, dg) for bn, st in forms for dg in (False, True)}
    return out | {("wgrad",) + tile for _, tile, _ in WGRAD_CASES}


def gen(*seed):
    return torch.Generator().manual_seed(hash(tuple(int(s) for s in seed)) % (2 ** 31))


def scale_of(t):
    """The 2^k the producers give a tensor with this abs-max."""
    return sp_scale_for(float(t.abs().max()))


class LinearInputs:
    """fp32 inputs of one Linear [rows, fin] -> [rows, fout]: x, w [fout, fin], bias, a gradient-sized g [rows, fout], and for the
    backward-data epilogue an addend of dx's own size and the operands (x0 [rows, 32], w0 [fin, 32], b0) of a small forward whose sp
    ReLU output [rows, fin] is the mask."""

    def __init__(self, rows, fin, fout):
        g = gen(rows, fin, fout)
        self.shape = (rows, fin, fout)
        self.x = torch.randn(rows, fin, generator=g) * 3.0
        self.w = torch.randn(fout, fin, generator=g) / fin ** 0.5
        self.b = torch.randn(fout, generator=g)
        self.g = torch.randn(rows, fout, generator=g) * 1e-3
        self.addend = torch.randn(rows, fin, generator=g) * 1e-3
        self.x0 = torch.randn(rows, 32, generator=g)
        self.w0 = torch.randn(fin, 32, generator=g) / 32 ** 0.5
        self.b0 = torch.randn(fin, generator=g) * 0.1


@functools.lru_cache(maxsize=4)
def linear_inputs(rows, fin, fout):
    return LinearInputs(rows, fin, fout)


def lin_out_sinv(fin, x_sinv, w_sinv, bias_absmax):
    """bf16_tile.h's bound-derived scale of an sp result, in fp32 as the epilogue evaluates it: (bound, 2^-k)."""
    osc = np.float32(x_sinv) * np.float32(w_sinv)
    bound = np.float32(fin) * np.float32(2.0 ** 30) * osc + np.float32(bias_absmax)
    return bound, np.float32(1.0) / np.float32(sp_scale_for(bound))


# ---------------------------------------------------------------- split_colsum
COLSUM_ROWS = (1, 63, 64, 200, 1100)
COLSUM_COLS = (32, 96, 512)
COLSUM_MAGS = (1e-6, 1.0, 1e5)


def colsum_inputs(rows, cols, mag):
    """(g, db0): a gradient of magnitude `mag` (0: all zeros) and a non-zero starting db of the column sums' size."""
    gn = gen(rows, cols, int(np.log10(mag)) + 20 if mag else 0)
    g = torch.randn(rows, cols, generator=gn) * mag if mag else torch.zeros(rows, cols)         # (randn * 0 would hold -0.0)
    return g, torch.randn(cols, generator=gn) * (mag * rows ** 0.5 if mag else 1.0)


def colsum_bound(g, db0=None):
    """(ceil(rows / 64) + 64) * 2^-24 * (sum_r |g[r][c]| + |db0[c]|): a row lane adds ceil(rows / 64) values in turn, one thread per
    column then adds the 64 lanes onto db0 (or 0) in turn - every value passes at most that many fp32 additions."""
    rows = g.shape[0]
    s = g.double().abs().sum(0) + (db0.double().abs() if db0 is not None else 0.0)
    return (-(-rows // 64) + 64) * U * s


def colsum_f32(g, db0=None):
    """split_colsum_kernel's summation in numpy float32: lane rl adds rows rl, rl + 64, ..; the lanes are added onto db0 in order."""
    a = g.numpy().astype(np.float32)
    rows, cols = a.shape
    lanes = np.zeros((64, cols), dtype=np.float32)
    for r in range(rows):
        lanes[r % 64] += a[r]
    t = db0.numpy().astype(np.float32).copy() if db0 is not None else np.zeros(cols, dtype=np.float32)
    for lane in range(64):
        t += lanes[lane]
    return t


# ---------------------------------------------------------------- absmax_multi
ABSMAX_GRID = 512 * 256 * 8          # elements one pass of the largest grid covers: beyond it the grid-stride loop runs again
ABSMAX_COUNTS = (0, 1, 255, 257, 300001, ABSMAX_GRID + 151425, 4096, 2048)       # the seventh all zeros; the sixth 1 200 001


def absmax_tensors():
    """Eight fp32 vectors: [0] is passed with a zero count; [4] holds its maximum at the first element, [5] - longer than one pass of
    the grid - a NEGATIVE one at the last; [6] is all zeros."""
    out = []
    for i, n in enumerate(ABSMAX_COUNTS):
        v = torch.randn(max(n, 8), generator=gen(i, n)) * (10.0 ** (i - 3))
        if i == 4:
            v[0] = float(v.abs().max()) * 1.5
        if i == 5:
            v[-1] = -float(v.abs().max()) * 1.5
        if i == 6:
            v.zero_()
        out.append(v)
    return out


# ---------------------------------------------------------------- fuse_build_split / fuse_unbuild
def directed_pairs(views):
    vi, vj = [], []
    for i, j in itertools.combinations(range(views), 2):
        vi += [i, j]
        vj += [j, i]
    return vi, vj


def rotations(n, g):
    q, _ = torch.linalg.qr(torch.randn(n, 3, 3, generator=g, dtype=torch.float64))
    return q.float().contiguous()


def rows_of(idx, B):
    """int32 [len(idx) * B]: row (d, b) -> idx[d] * B + b."""
    return (torch.tensor(idx, dtype=torch.int32)[:, None] * B + torch.arange(B, dtype=torch.int32)[None, :]).reshape(-1).contiguous()


BUILD_SIZES = ((8, 8, 1.0), (64, 16, 1e-3), (2056, 8, 1e3), (64, 688, 1.0))         # cf, nvec, magnitude; 257 image chunks; 258 feature chunks
BUILD_V, BUILD_B = 3, 5
SQRT3_F32 = np.float32(1.7320509)


class BuildInputs:
    """img [V B, cf], F [D B, 3 nvec], rel [D B, 3, 3] and the row tables of heads.py: the image row of direction d's source view,
    the partner direction's feature row for xf, the direction's own for xh."""

    def __init__(self, cf, nvec, mag):
        V, B = BUILD_V, BUILD_B
        g = gen(cf, nvec, 7)
        vi, _ = directed_pairs(V)
        D = len(vi)
        self.rows, self.cf, self.nvec = D * B, cf, nvec
        self.img = torch.randn(V * B, cf, generator=g).abs() * mag
        self.F = torch.randn(self.rows, 3 * nvec, generator=g) * (mag * 7)
        self.rel = rotations(self.rows, g)
        self.row_img, self.partner, self.ident = rows_of(vi, B), rows_of([d ^ 1 for d in range(D)], B), rows_of(list(range(D)), B)
        self.am_img, self.am_feat = np.float32(float(self.img.abs().max())), np.float32(float(self.F.abs().max()))
        # both scales in fp32, as the kernel evaluates them
        self.sf = sp_scale_for(max(self.am_img, SQRT3_F32 * self.am_feat))
        self.sh = sp_scale_for(max(self.am_img, self.am_feat))

    def rotated(self, rel):
        """(float64 rel @ F[partner] [rows, 3 nvec], sum_j |r_aj f_j| of the same shape)."""
        f = self.F.double()[self.partner.long()].view(self.rows, 3, self.nvec)
        r = (self.rel.double() if rel else torch.eye(3, dtype=torch.float64).expand(self.rows, 3, 3))
        return (torch.einsum("mij,mjk->mik", r, f).reshape(self.rows, -1), torch.einsum("mij,mjk->mik", r.abs(), f.abs()).reshape(self.rows, -1))

    def rotated_f32(self):
        """The kernel's three-term expression in numpy float32, without contraction: r0 f0 + r1 f1 + r2 f2, left to right."""
        f = self.F.numpy()[self.partner.long().numpy()].reshape(self.rows, 3, self.nvec)
        r = self.rel.numpy()
        out = np.empty((self.rows, 3, self.nvec), dtype=np.float32)
        for a in range(3):
            out[:, a] = (r[:, a, 0:1] * f[:, 0] + r[:, a, 1:2] * f[:, 1]) + r[:, a, 2:3] * f[:, 2]
        return out.reshape(self.rows, -1)


@functools.lru_cache(maxsize=None)
def build_inputs(cf, nvec, mag):
    return BuildInputs(cf, nvec, mag)


def build_bound(want, absterms, sinv):
    """3 * 2^-24 * sum_j |r_aj f_j| (two products and two additions deep at most, either contraction) + the sp format's
    2^-23 |want| + 2^-25 stored units."""
    return 3 * U * absterms + 2.0 ** -23 * want.abs() + 2.0 ** -25 * sinv


UNBUILD_SIZES = ((4, 4), (64, 16), (1028, 260))          # cf, nvec: 257 float4 of the image part, 260 > 256 feature columns
UNBUILD_VB = ((3, 5), (4, 1))                            # S * B = 30: the last workgroup of 4 rows holds 2; one row per segment
UNBUILD_MODES = ("both", "dxn_only", "dxh_only")         # dxn only: iteration 0, segments = views


class UnbuildCase:
    """dxh, dxn [D B, cf + 3 nvec], rel, the segment tables, a starting da, and float64 dF / da with the count and the absolute sum
    of the fp32 terms behind every element."""

    def __init__(self, V, B, cf, nvec, mode, rel, accumulate):
        g = gen(V, B, cf, nvec, len(mode), rel, accumulate)
        vi, vj = directed_pairs(V)
        D = len(vi)
        self.V, self.B, self.D, self.cf, self.nvec = V, B, D, cf, nvec
        kin = cf + 3 * nvec
        self.dxh = torch.randn(D * B, kin, generator=g) if mode != "dxn_only" else None
        self.dxn = torch.randn(D * B, kin, generator=g) * 0.5 if mode != "dxh_only" else None
        self.rel = rotations(D * B, g) if rel else None
        self.vi = vi
        self.seg = vj if mode == "dxn_only" else [d ^ 1 for d in range(D)]         # the source view / the partner direction
        self.S = V if mode == "dxn_only" else D
        self.da0 = torch.randn(V, B, cf, generator=g)
        self.accumulate = accumulate
        # dF
        dF = torch.zeros(self.S, B, 3, nvec, dtype=torch.float64)
        dF_abs, dF_terms = torch.zeros_like(dF), torch.zeros(self.S)
        if self.dxh is not None:
            h = self.dxh.double()[:, cf:].view(D, B, 3, nvec)
            dF += h
            dF_abs += h.abs()
            dF_terms += 1
        if self.dxn is not None:
            gn = self.dxn.double()[:, cf:].view(D, B, 3, nvec)
            r = self.rel.double().view(D, B, 3, 3) if rel else torch.eye(3, dtype=torch.float64).expand(D, B, 3, 3)
            back, back_abs = torch.einsum("dbji,dbjk->dbik", r, gn), torch.einsum("dbji,dbjk->dbik", r.abs(), gn.abs())
            for d in range(D):
                dF[self.seg[d]] += back[d]
                dF_abs[self.seg[d]] += back_abs[d]
                dF_terms[self.seg[d]] += 3 if rel else 1
        self.dF, self.dF_bound = dF, dF_terms.view(-1, 1, 1, 1) * U * dF_abs
        # da
        da = self.da0.double().clone() if accumulate else torch.zeros(V, B, cf, dtype=torch.float64)
        da_abs, da_terms = da.abs(), torch.full((V,), 1.0 if accumulate else 0.0)
        for d in range(D):
            for t in (self.dxh, self.dxn):
                if t is not None:
                    part = t.double()[:, :cf].view(D, B, cf)[d]
                    da[vi[d]] += part
                    da_abs[vi[d]] += part.abs()
                    da_terms[vi[d]] += 1
        self.da, self.da_bound = da, da_terms.view(-1, 1, 1) * U * da_abs

    def f32(self):
        """fuse_unbuild_kernel's sums in numpy float32, in its order, without contraction: (dF, da)."""
        D, B, cf, nvec = self.D, self.B, self.cf, self.nvec
        dF = np.zeros((self.S, B, 3, nvec), dtype=np.float32)
        if self.dxh is not None:
            dF += self.dxh.numpy()[:, cf:].reshape(D, B, 3, nvec)
        if self.dxn is not None:
            gn = self.dxn.numpy()[:, cf:].reshape(D, B, 3, nvec)
            for d in range(D):
                if self.rel is not None:
                    r = self.rel.numpy().reshape(D, B, 3, 3)[d]
                    for a in range(3):
                        dF[self.seg[d], :, a] += (r[:, 0, a:a + 1] * gn[d, :, 0] + r[:, 1, a:a + 1] * gn[d, :, 1]) + r[:, 2, a:a + 1] * gn[d, :, 2]
                else:
                    dF[self.seg[d]] += gn[d]
        da = self.da0.numpy().copy() if self.accumulate else np.zeros((self.V, B, cf), dtype=np.float32)
        for d in range(D):
            for t in (self.dxh, self.dxn):
                if t is not None:
                    da[self.vi[d]] += t.numpy()[:, :cf].reshape(D, B, cf)[d]
        return dF, da


def unbuild_cases():
    """(V, B, cf, nvec, mode, rel, accumulate): every mode x rel x accumulate at the middle size and V = 3; the other sizes and
    V = 4, B = 1 with both gradients, rel and accumulate alternating."""
    out = [(3, 5, 64, 16, mode, rel, acc) for mode in UNBUILD_MODES for rel in (True, False) for acc in (False, True)]
    for cf, nvec in ((4, 4), (1028, 260)):
        out += [(3, 5, cf, nvec, mode, mode != "dxh_only", mode == "both") for mode in UNBUILD_MODES]
    out += [(4, 1, cf, nvec, mode, mode != "dxn_only", mode != "both") for cf, nvec in UNBUILD_SIZES for mode in UNBUILD_MODES]
    return out
