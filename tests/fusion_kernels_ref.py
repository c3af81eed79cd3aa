"""float64 references, written from the definitions, of the small kernels of csrc/fusion.hip and csrc/pool.hip (the fuser / head
operand builders, the IntensityBatchNorm scale walk, segment sums, the <= 4-wide Linear, the losses and the pools), and the case
tables tests/test_fusion_kernels_gpu.py parametrises over.  No GPU and no library call in here: tests/test_fusion_kernels_cpu.py
ties every function to the oracle (oracle/restatement.py, itself pinned to the reference's fixtures) or to autograd, and asserts
the preconditions of the case tables on these references alone.

Layouts are the kernels' (heads.py): directions d = 2p (i <- j), 2p + 1 (j <- i) of the p-th unordered pair; image features
[V, B, cf]; feature tensors [S, B, 3, nvec] (S = views for the lifted features, = directions for an iteration's output); relative
rotations [D, B, 3, 3]; operand rows (d, b)."""
import itertools
import math

import torch
import torch.nn.functional as F

NVEC = 512                                  # the host always passes arch.NUM_FEAT_VEC
IBN_MOMENTUM, IBN_EPS = 0.05, 1e-4          # IntensityBatchNorm's defaults (rot_mv.py:14), what heads.py passes
DEG = 180.0 / math.pi


def randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float32)


def rand(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float32)


def directed_pairs(views):
    """(vi, vj): direction d reads view vi[d]'s image feature and view vj[d]'s partner feature."""
    vi, vj = [], []
    for i, j in itertools.combinations(range(views), 2):
        vi += [i, j]
        vj += [j, i]
    return vi, vj


def rotations(n, seed, dtype=torch.float32):
    """n proper rotation matrices [n, 3, 3] (float32: roundings of the float64 ones): Ry(yaw) Rx(-pitch) of angles within +-0.5."""
    a = (rand((n, 2), seed).double() - 0.5)
    p, y = -a[:, 0], a[:, 1]
    one, zero = torch.ones_like(p), torch.zeros_like(p)
    rx = torch.stack([one, zero, zero, zero, p.cos(), -p.sin(), zero, p.sin(), p.cos()], 1).view(-1, 3, 3)
    ry = torch.stack([y.cos(), zero, y.sin(), zero, one, zero, -y.sin(), zero, y.cos()], 1).view(-1, 3, 3)
    return (ry @ rx).to(dtype)


def relative_rotation(rot, vi, vj):
    """rot [B, V, 3, 3] -> rel [D, B, 3, 3] = rot[:, vi[d]] @ rot[:, vj[d]]^T   (rot_mv.py:193-194)."""
    rot = rot.double()
    return torch.stack([rot[:, i] @ rot[:, j].transpose(-1, -2) for i, j in zip(vi, vj)])


# ---------------------------------------------------------------- operand builders
def _rotated(feat, rel, src_of):
    f = feat.double()[list(src_of)]                                   # [D, B, 3, nvec]
    return f if rel is None else rel.double() @ f


def rotcat(img_feat, feat, rel, view_of, src_of):
    """ImageFeatFuser's input (rot_mv.py:44-50 on the rotated partner feature of :234-239; rel None = ignore_rotmat :226-232, and
    the gaze head's input :249-254): x[d, b] = [ img_feat[view_of[d], b] | (rel[d, b] @ feat[src_of[d], b]) flattened axis-major ]."""
    return torch.cat([img_feat.double()[list(view_of)], _rotated(feat, rel, src_of).flatten(-2, -1)], -1)


def rotcat_bwd(dx, rel, src_of, sources, cf, nvec=NVEC):
    """Gradient of rotcat's feature part, per direction: dfeat[src_of[d], b] = rel[d, b]^T @ dx[d, b, cf:cf + 3 nvec] (src_of must
    be a permutation: the kernel writes, it does not sum - heads.py sums shared sources with segment_sum afterwards)."""
    assert sorted(src_of) == list(range(sources))
    g = dx.double()[..., cf:cf + 3 * nvec].reshape(dx.shape[0], dx.shape[1], 3, nvec)
    g = g if rel is None else rel.double().transpose(-1, -2) @ g
    out = torch.empty_like(g)
    out[list(src_of)] = g
    return out


def rotcat_ext(img_feat, feat, rel_apply, rel_append, view_of, src_of, ld):
    """ImageRotmatFeatFuser's input (encode_rotmat, rot_mv.py:53-69,219-225), rows padded with zeros to ld:
    [ img_feat | rel_apply @ feat (feat itself when rel_apply is None) | rel_append flattened, 9 entries (zeros when None) | 0 .. ]."""
    x = rotcat(img_feat, feat, rel_apply, view_of, src_of)
    D, B, used = x.shape
    tail = torch.zeros(D, B, ld - used, dtype=torch.float64)
    if rel_append is not None:
        tail[..., :9] = rel_append.double().flatten(-2, -1)
    return torch.cat([x, tail], -1)


def rotcat_ext_bwd(dx, rel, src_of, sources, cf, nvec=NVEC):
    """As rotcat_bwd on rows of leading dimension ld = dx.shape[-1]; the 9 appended entries and the padding carry no gradient
    to the features."""
    return rotcat_bwd(dx, rel, src_of, sources, cf, nvec)


def paircat(a, feat, rel, scales, view_of, src_of):
    """RotFeatFuser's input (share_feature, rot_mv.py:72-86) given the two normalisers' scales, and with scales = rel = None the
    gaze head's input of that variant (:241-247): x[d, b] = cat([a[view_of[d], b] * s[2d], (rel @ feat[src_of[d], b]) * s[2d + 1]],
    dim=-1) flattened axis-major, i.e. [axis][0:nvec | nvec:2 nvec]."""
    a0 = a.double()[list(view_of)]
    f = _rotated(feat, rel, src_of)
    if scales is not None:
        s = scales.double().view(-1, 2, 1, 1, a.shape[-1])
        a0, f = a0 * s[:, 0], f * s[:, 1]
    return torch.cat([a0, f], -1).flatten(-2, -1)


def paircat_bwd(dx, rel, scales, src_of, sources, nvec=NVEC):
    """dx [D, B, 6 nvec] -> (da_dir [D, B, 3, nvec] = s[2d] * dx's first halves, dfeat[src_of[d]] = rel^T @ (s[2d + 1] * second halves))."""
    assert sorted(src_of) == list(range(sources))
    g = dx.double().reshape(dx.shape[0], dx.shape[1], 3, 2 * nvec)
    ga, gf = g[..., :nvec], g[..., nvec:]
    if scales is not None:
        s = scales.double().view(-1, 2, 1, 1, nvec)
        ga, gf = ga * s[:, 0], gf * s[:, 1]
    gf = gf if rel is None else rel.double().transpose(-1, -2) @ gf
    out = torch.empty_like(gf)
    out[list(src_of)] = gf
    return ga.contiguous(), out


def ibn_call_variances(a, feat, view_of, src_of):
    """[2 D, nvec]: the biased batch variance of the column norms that each of the 2 D normaliser calls sees."""
    out = []
    for d in range(len(view_of)):
        for x in (a.double()[view_of[d]], feat.double()[src_of[d]]):
            out.append(torch.var(torch.norm(x, dim=-2), unbiased=False, dim=0))
    return torch.stack(out)


def ibn_scales(a, feat, view_of, src_of, running_mean, training, momentum=IBN_MOMENTUM, eps=IBN_EPS):
    """The IntensityBatchNorm walk of one iteration (rot_mv.py:13-32 called as :80-81 for direction 0, 1, ...): 2 D calls in
    sequence on ONE buffer - a[view_of[d]] then feat[src_of[d]] (the norm of a rotated column is the column's) - each, in training,
    FIRST moving running_mean towards sqrt(max(var, eps)) of the batch's column norms and THEN dividing by (running_mean + eps).
    Returns (scales [2 D, nvec], the buffer after the last call)."""
    rm = running_mean.double().reshape(-1).clone()
    var = ibn_call_variances(a, feat, view_of, src_of)
    scales = []
    for call in range(var.shape[0]):
        if training:
            rm = rm * (1 - momentum) + torch.sqrt(var[call].clamp_min(eps)) * momentum
        scales.append(1.0 / (rm + eps))
    return torch.stack(scales), rm


def ibn_scales_f32(a, feat, view_of, src_of, running_mean, momentum=IBN_MOMENTUM, eps=IBN_EPS):
    """The training walk in the kernel's number formats, in torch on the CPU: float32 norms, float64 batch variance rounded to
    float32, and the recurrence rm * (1 - momentum) + sd * momentum and 1 / (rm + eps) in float32.  Measures what float32 costs
    against ibn_scales (the recurrence carries each step's rounding into the next; it is not a statement about any kernel)."""
    f = torch.float32
    rm = running_mean.to(f).reshape(-1).clone()
    mom, e = torch.tensor(momentum, dtype=f), torch.tensor(eps, dtype=f)
    keep = torch.tensor(1.0, dtype=f) - mom
    scales = []
    for d in range(len(view_of)):
        for x in (a.to(f)[view_of[d]], feat.to(f)[src_of[d]]):
            norm = torch.sqrt((x * x).sum(-2))
            var = torch.var(norm.double(), unbiased=False, dim=0).to(f)
            rm = rm * keep + torch.sqrt(var.clamp_min(e)) * mom
            scales.append(1.0 / (rm + e))
    return torch.stack(scales), rm


def segment_sum(x, width, seg_of, segments, out0=None):
    """out[s, b, :width] = (out0[s, b] if accumulating) + sum over d with seg_of[d] == s of x[d, b, :width]."""
    out = torch.zeros(segments, x.shape[1], width, dtype=torch.float64) if out0 is None else out0.double().clone()
    for d, s in enumerate(seg_of):
        out[s] += x.double()[d, :, :width]
    return out


# ---------------------------------------------------------------- the <= 4-wide Linear of the gaze head
def skinny_fwd(x, w, bias):
    return F.linear(x.double(), w.double(), None if bias is None else bias.double())


def skinny_bwd(dy, x, w, mask, dw0=None, db0=None):
    """(dx = (dy @ w) * (mask > 0), dw = dy^T @ x (+ dw0), db = column sums of dy (+ db0))."""
    dy, x, w = dy.double(), x.double(), w.double()
    dx = dy @ w
    if mask is not None:
        dx = dx * (mask > 0).double()
    dw, db = dy.t() @ x, dy.sum(0)
    return dx, dw + (0 if dw0 is None else dw0.double()), db + (0 if db0 is None else db0.double())


# ---------------------------------------------------------------- losses
def pitchyaw_to_vector(py):
    s, c = torch.sin(py), torch.cos(py)
    return torch.stack([c[..., 0] * s[..., 1], s[..., 0], c[..., 0] * c[..., 1]], -1)


def angles(pred, gt):
    """Per-row angle in degrees (gaze_loss.py:42-52): acos(hardtanh(cosine_similarity(v(gt), v(pred), eps=1e-6)))."""
    sim = F.cosine_similarity(pitchyaw_to_vector(gt), pitchyaw_to_vector(pred), dim=-1, eps=1e-6)
    return torch.acos(F.hardtanh(sim, -1.0, 1.0)) * DEG


def angular_loss(pred, gt, row_weight):
    """(theta [n] in degrees, loss = row_weight * sum theta, dloss/dpred by float64 autograd)."""
    p = pred.double().clone().requires_grad_(True)
    theta = angles(p, gt.double())
    loss = theta.sum() * row_weight
    loss.backward()
    return theta.detach(), loss.detach(), p.grad


def angular_loss_multi(pred, gt, weights, dirs, batch):
    """pred [iters, dirs * batch, 2], gt [dirs * batch, 2]: loss = sum_{it, d} weights[it * dirs + d] * mean_b theta[it, d, b]
    (stereo_loss.py:46-54 inside :65-84 over every direction), and its gradient."""
    p = pred.double().clone().requires_grad_(True)
    iters = p.shape[0]
    theta = angles(p, gt.double()[None].expand_as(p)).view(iters, dirs, batch)
    w = torch.as_tensor(list(weights), dtype=torch.float64).view(iters, dirs)
    loss = (theta.mean(-1) * w).sum()
    loss.backward()
    return loss.detach(), p.grad


def lp_loss(pred, label, p):
    """mean |pred - label|^p over all elements (gaze_loss.py:56-64) and its gradient (torch.abs: zero at 0)."""
    a = pred.double().clone().requires_grad_(True)
    loss = ((a - label.double()).abs() ** p).mean()
    loss.backward()
    return loss.detach(), a.grad


# ---------------------------------------------------------------- pools
def maxpool(x_nchw, dy_nchw=None):
    """MaxPool2d(3, 2, 1) by ATen: (y float32, the kernel's argmax code kh * 3 + kw of ATen's winner - its flat input index
    converted -, dx by float64 autograd or None).  All in NHWC, the kernels' layout."""
    y, idx = F.max_pool2d(x_nchw, 3, 2, 1, return_indices=True)
    n, c, ho, wo = y.shape
    w = x_nchw.shape[3]
    oy = torch.arange(ho).view(1, 1, ho, 1)
    ox = torch.arange(wo).view(1, 1, 1, wo)
    kh, kw = idx // w - (oy * 2 - 1), idx % w - (ox * 2 - 1)
    assert int(kh.min()) >= 0 and int(kh.max()) <= 2 and int(kw.min()) >= 0 and int(kw.max()) <= 2
    code = (kh * 3 + kw).to(torch.uint8)
    dx = None
    if dy_nchw is not None:
        xr = x_nchw.double().requires_grad_(True)
        F.max_pool2d(xr, 3, 2, 1).backward(dy_nchw.double())
        dx = xr.grad.permute(0, 2, 3, 1).contiguous()
    return y.permute(0, 2, 3, 1).contiguous(), code.permute(0, 2, 3, 1).contiguous(), dx


def maxpool_tie_fraction(x_nchw):
    """Share of the pooling windows whose maximum is attained more than once."""
    n, c, h, w = x_nchw.shape
    win = F.unfold(F.pad(x_nchw.double(), (1, 1, 1, 1), value=float("-inf")), 3, 1, 0, 2).view(n, c, 9, -1)
    ties = (win == win.max(2, keepdim=True).values).sum(2) > 1
    return float(ties.double().mean())


def avgpool(x):
    """x [n, hw, c] -> [n, c]."""
    return x.double().mean(1)


def avgpool_bwd(dy, hw):
    return (dy.double() / hw)[:, None, :].expand(dy.shape[0], hw, dy.shape[1]).contiguous()


# ---------------------------------------------------------------- case tables (the smallest shapes that reach each edge)
# rotcat_fwd / rotcat_bwd / relative_rotation: (V, B, cf, rel given, source table); cf = 2048: cf / 4 > 256, the copy loop's
# second trip.  "view": iteration 0 (the partner VIEW's lifted feature), "partner": direction d ^ 1 of the previous iteration.
ROTCAT_CASES = [(V, 5, cf, use_rel, src) for V in (3, 4) for cf in (512, 2048) for use_rel in (True, False) for src in ("view", "partner")]

# rotcat_ext_fwd / bwd: (V, B, cf, ld, rel_apply given, rel_append given).  512 + 3 * 512 + 9 = 2057 -> ld 2060 (3 zero columns);
# ld 2316: 268 tail columns > 256 + 9, the tail loop's second trip.
ROTCAT_EXT_CASES = [(3, 5, 512, ld, ap, ad) for ld in (2060, 2316) for ap in (False, True) for ad in (False, True)] + [(4, 3, 2048, 3596, False, True)]

# ibn_scales + paircat: (V, B, training, source table)
IBN_CASES = [(V, B, tr, ("view", "partner")[(V + B + tr) % 2]) for V in (2, 3, 4) for B in (1, 5, 33) for tr in (True, False)]
# The bar on ibn_scales' scales.  1e-6 (the builders') does not hold for a correct float32 walk: each call's rm * 0.95 + sd * 0.05
# carries the roundings of the calls before it, and 1.f - momentum is itself rounded, so after 2 D = 24 calls the walk restated in
# float32 in torch on the CPU (ibn_scales_f32) is 1.10e-6 of the largest scale away from the float64 one (2e-7 at D = 2, 5e-7 at
# D = 6; tests/test_fusion_kernels_cpu.py measures it over the table and holds it to a quarter of this bar).  4 x that CPU figure:
IBN_SCALES_BAR = 4.4e-6
IBN_CLAMPED_EVERY = 4                       # columns k % 4 == 0: every batch row has the same column norm (var < eps: clamped)

# segment_sum: (V, B, cf, segments, accumulate): row_stride = cf + 3 nvec, width = cf, seg_of = vi (values < V): segment V is fed
# by no direction; 5 * 5 * 128 = 3200 accesses is no multiple of 256
SEGSUM_CASES = [(4, 5, 512, 5, False), (4, 5, 512, 5, True), (3, 33, 2048, 4, True), (2, 1, 512, 3, False)]

# axpby / scale_by: the grid is capped at 4096 workgroups of 256
STREAM_NS = [1, 255, 257, 4096 * 256 + 257]

# linear_skinny: (rows, k, nout); 520 * 512 > 1024 * 256: the dx kernel's second grid-stride trip
SKINNY_CASES = [(1, 64, 1), (3, 100, 3), (37, 512, 2), (5, 514, 4), (520, 512, 2)]

ANGULAR_NS = [1, 255, 257, 700]
ANGULAR_MULTI_CASES = [(3, 2, 3), (3, 6, 5), (3, 56, 2), (1, 512, 1)]          # (iters, dirs, batch)
LP_NS = [1, 257, 700]

MAXPOOL_CASES = [(1, 1, 1, 4), (2, 2, 3, 4), (3, 15, 17, 64), (1, 8, 8, 260)]    # (n, h, w, c)
AVGPOOL_CASES = [(1, 1, 4), (5, 4, 512), (3, 49, 2048), (7, 49, 36)]             # (n, hw, c)


def src_table(V, kind):
    """(src_of, number of source rows S) of a case's source table."""
    vi, vj = directed_pairs(V)
    D = len(vi)
    if kind == "view":
        return vj, V
    return ([d ^ 1 for d in range(D)] if kind == "partner" else list(range(D))), D


def rotcat_inputs(V, B, cf, seed=0):
    vi, vj = directed_pairs(V)
    D = len(vi)
    rot = rotations(B * V, 11 + seed).view(B, V, 3, 3)
    return {"vi": vi, "vj": vj, "D": D, "rot": rot, "rel": relative_rotation(rot, vi, vj).float(), "img": randn((V, B, cf), 12 + seed),
            "lifted": randn((V, B, 3, NVEC), 13 + seed), "feats": randn((D, B, 3, NVEC), 14 + seed)}


def ibn_inputs(V, B, kind):
    """a [V, B, 3, nvec], the source features and a running_mean in (0.5, 1.5).  Columns k % IBN_CLAMPED_EVERY == 0 of every
    tensor have ONE norm per (row of the leading axis, column) across the batch - different vectors, the same length up to
    float32 rounding -, so their batch variance is ~1e-14 < eps; the other columns are N(0, 1) vectors (variance ~0.4)."""
    vi, vj = directed_pairs(V)
    D = len(vi)
    src_of, S = src_table(V, kind)

    def make(lead, seed):
        x = randn((lead, B, 3, NVEC), seed).double()
        length = 0.5 + rand((lead, 1, 1, NVEC), seed + 1).double()
        fixed = x / torch.norm(x, dim=-2, keepdim=True) * length
        cl = torch.arange(NVEC) % IBN_CLAMPED_EVERY == 0
        return torch.where(cl, fixed, x).float()
    return {"vi": vi, "vj": vj, "D": D, "src_of": src_of, "S": S, "a": make(V, 100 * V + B), "feat": make(S, 100 * V + B + 7),
            "rm": 0.5 + rand((NVEC,), 31 * V + B), "rel": relative_rotation(rotations(B * V, V + B).view(B, V, 3, 3), vi, vj).float()}


def _angular_offsets(n, seed):
    """[n, 2] offsets in (pitch, yaw) of length 0.3 .. 0.5 rad in a random direction."""
    phi, m = rand((n,), seed) * (2 * math.pi), 0.3 + 0.2 * rand((n,), seed + 1)
    return torch.stack([m * torch.sin(phi), m * torch.cos(phi)], 1)


def angular_inputs(n, seed=0):
    """(pred, gt) [n, 2]: labels with |pitch| < 0.7, |yaw| < 1; the prediction 0.3 .. 0.5 rad away in (pitch, yaw)."""
    gt = (rand((n, 2), 40 + seed) * 2 - 1) * torch.tensor([0.7, 1.0])
    return (gt + _angular_offsets(n, 41 + seed)).contiguous(), gt.contiguous()


def angular_multi_inputs(iters, dirs, batch):
    """(pred [iters, dirs * batch, 2], gt [dirs * batch, 2]): every iteration's prediction its own offset from the one label."""
    _, gt = angular_inputs(dirs * batch, 5)
    return torch.stack([gt + _angular_offsets(dirs * batch, 60 + 10 * it) for it in range(iters)]).contiguous(), gt


def maxpool_input(n, h, w, c):
    """ReLU of N(0, 1) values rounded to halves (NCHW float32): zeros and repeated positive values, so ties for a window's maximum are common."""
    return F.relu(torch.round(randn((n, c, h, w), 7 * n + h + w + c) * 2) / 2)
