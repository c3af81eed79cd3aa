"""Host arithmetic behind tests/test_bn_forms_{cpu,gpu}.py: float64 restatements of what csrc/bn.hip computes, written from the
documented formats and formulas - not from the library - and the case tables both test files share, with the answers the
host-only plan query (mvg_bn_plan_query) must give on 256 CUs.

  write_partials    the conv epilogue's statistics format: per rows_per_partial rows the sum and the sum of squares centred on
                    the partial's own mean, both rounded to fp32; a ragged last partial; surplus slots hold NaN
  merge_partials    those fp32 partials merged in float64 (Chan) to mean / invstd / scale / shift, and the running statistics
                    updated in group order with the unbiased variance - the fp32 recurrence BatchNorm2d runs
  apply_ref, train_bwd_ref, eval_bwd_ref, stem_tail_ref
                    the element passes in float64 (the stem tail by autograd through F.batch_norm / F.max_pool2d)
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
MOMENTUM = 0.1
FP32, BF16, SP = 0, 1, 2                                        # _lib.BN_ELEM_*
ELEM_NAMES = {FP32: "fp32", BF16: "bf16", SP: "sp"}
WALK_GROUPS, ALL_GROUPS, PER_GROUP = 0, 1, 2                    # _lib.BN_MERGE_*
NAN = float("nan")


def randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


# ---------------------------------------------------------------- statistics: partial writer and merge
def write_partials(x, rows_per_partial, slots=None):
    """x [G, rows, C] fp32 -> [G, slots, 2, C] fp32: partial p covers rows p * rows_per_partial ... of its group and holds
    (sum, sum of (x - the partial's own mean)^2), evaluated in float64 and rounded once.  slots > the partials the rows need:
    the surplus slots are NaN (the merge must not read them)."""
    G, rows, C = x.shape
    rpp = int(rows_per_partial)
    valid = -(-rows // rpp)
    slots = valid if slots is None else int(slots)
    assert slots >= valid
    out = torch.full((G, slots, 2, C), NAN, dtype=torch.float32)
    xd = x.double()
    full = rows // rpp
    if full:
        blk = xd[:, :full * rpp].reshape(G, full, rpp, C)
        s = blk.sum(2)
        out[:, :full, 0] = s.float()
        out[:, :full, 1] = ((blk - s[:, :, None] / rpp) ** 2).sum(2).float()
    if valid > full:
        tail = xd[:, full * rpp:]
        s = tail.sum(1)
        out[:, full, 0] = s.float()
        out[:, full, 1] = ((tail - s[:, None] / tail.shape[1]) ** 2).sum(1).float()
    return out


def merge_partials(stats, rows, rows_per_partial, gamma, beta, running_mean=None, running_var=None, momentum=MOMENTUM, eps=EPS):
    """The fp32 partials of write_partials merged in float64.  Returns float64 mean, invstd, scale, shift [G, C]; the unbiased
    variance [G, C]; and - given running statistics - their fp32 values after one update per group, in group order:
    r = (1 - momentum) r + momentum fp32(statistic), every operation rounded to fp32 (numpy float32)."""
    st = stats.double()
    G, P, _, C = st.shape
    rpp = int(rows_per_partial)
    valid = min(-(-rows // rpp), P)
    cnt = torch.full((valid,), float(rpp), dtype=torch.float64)
    cnt[-1] = min(rows - (valid - 1) * rpp, rpp)
    s, q = st[:, :valid, 0], st[:, :valid, 1]
    S, Q = s.sum(1), q.sum(1)
    n = float(rows)
    mean = S / n
    # Chan: the partials' centred squares + the between-partials term, as sum cnt_p (mean_p - mean)^2: of the size of the variance
    # (sum s_p^2 / cnt_p - S mean is the same number, but float64 keeps only 2^-53 of n mean^2 of it)
    between = (cnt[None, :, None] * (s / cnt[None, :, None] - mean[:, None]) ** 2).sum(1)
    m2 = torch.clamp(Q + between, min=0.0)
    var = m2 / n
    invstd = 1.0 / torch.sqrt(var + float(np.float32(eps)))
    scale = gamma.double()[None] * invstd
    shift = beta.double()[None] - mean * scale
    unbiased = m2 / (n - 1.0) if rows > 1 else var
    out = {"mean": mean, "invstd": invstd, "scale": scale, "shift": shift, "unbiased": unbiased, "rm": None, "rv": None}
    m32 = np.float32(momentum)
    keep = np.float32(1.0) - m32
    for key, start, stat in (("rm", running_mean, mean), ("rv", running_var, unbiased)):
        if start is None:
            continue
        r = start.numpy().astype(np.float32).copy()
        for g in range(G):
            r = keep * r + m32 * stat[g].numpy().astype(np.float32)
        out[key] = torch.from_numpy(r)
    return out


def ulps(got, ref64):
    """|got - ref| in units of the fp32 spacing at ref (got fp32, ref float64), elementwise maximum."""
    ref32 = ref64.float()
    sp = torch.from_numpy(np.spacing(np.abs(ref32.numpy()).astype(np.float32))).double()
    return float(((got.double().cpu() - ref64).abs() / sp).max())


# ---------------------------------------------------------------- element passes in float64
def group_stats(y, eps=EPS):
    """Batch statistics per (group, channel) of y [G, rows, C] in float64: mean, invstd (biased variance)."""
    yd = y.double()
    mean = yd.mean(1)
    var = ((yd - mean[:, None]) ** 2).mean(1)
    return mean, 1.0 / torch.sqrt(var + eps)


def apply_ref(y, scale, shift, residual=None, res_affine=None, relu=False):
    """out = [relu](y scale + shift [+ residual | residual rs + rh]); scale, shift [G, C].  Returns (pre-ReLU, out) in float64."""
    pre = y.double() * scale.double()[:, None] + shift.double()[:, None]
    if residual is not None:
        r = residual.double()
        if res_affine is not None:
            r = r * res_affine[0].double()[:, None] + res_affine[1].double()[:, None]
        pre = pre + r
    return pre, (torch.clamp(pre, min=0.0) if relu else pre)


def mask_bytes(on, per):
    """The ReLU mask bytes of bn_apply_bits: one byte per 16-byte access (`per` elements: 4 in fp32 / sp, 8 in bf16), bit k =
    element k of the access came out > 0."""
    w = torch.tensor([1 << k for k in range(per)], dtype=torch.int32)
    return (on.reshape(-1, per).to(torch.int32) * w).sum(1).to(torch.uint8)


def train_bwd_ref(go, y, mean, invstd, gamma, mask=None):
    """Training-mode backward of one unit, float64: dz = go masked; s1 = sum dz, s2 = sum dz xhat per (group, channel);
    dgamma = sum_g s2, dbeta = sum_g s1; dy = gamma invstd (dz - s1 / n - xhat s2 / n)."""
    n = y.shape[1]
    xhat = (y.double() - mean.double()[:, None]) * invstd.double()[:, None]
    dz = go.double() if mask is None else go.double() * mask.double()
    s1, s2 = dz.sum(1), (dz * xhat).sum(1)
    dy = gamma.double()[None, None] * invstd.double()[:, None] * (dz - s1[:, None] / n - xhat * s2[:, None] / n)
    return {"dz": dz, "s1": s1, "s2": s2, "dgamma": s2.sum(0), "dbeta": s1.sum(0), "dy": dy}


def eval_bwd_ref(go, y, gamma, running_mean, running_var, eps=EPS, mask=None):
    """Eval-mode backward: xhat on the running statistics; dy = gamma invstd_r dz; dbeta = sum dz, dgamma = sum dz xhat over
    every row of every group."""
    isr = 1.0 / torch.sqrt(running_var.double() + eps)
    xhat = (y.double() - running_mean.double()) * isr
    dz = go.double() if mask is None else go.double() * mask.double()
    return {"dz": dz, "dy": gamma.double() * isr * dz, "dgamma": (dz * xhat).sum((0, 1)), "dbeta": dz.sum((0, 1))}


def stem_tail_ref(y, gamma, beta, gp_of, train=True, running_mean=None, running_var=None, eps=EPS):
    """BatchNorm -> ReLU -> MaxPool2d(3, 2, 1) of y [G, N, C, H, W] by autograd in float64, one BatchNorm call per group.
    gp_of(shape) gives the pooled gradient [G, N, C, ho, wo].  Returns pooled, dy (both NCHW), dgamma, dbeta, gp."""
    yr = y.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm = None if train else running_mean.double()
    rv = None if train else running_var.double()
    pooled = torch.stack([F.max_pool2d(F.relu(F.batch_norm(yr[g], rm, rv, gr, br, train, MOMENTUM, eps)), 3, 2, 1)
                          for g in range(y.shape[0])])
    gp = gp_of(tuple(pooled.shape))
    pooled.backward(gp.double())
    return {"pooled": pooled.detach(), "dy": yr.grad, "dgamma": gr.grad, "dbeta": br.grad, "gp": gp}


def dy_scale_inverse(gamma, invstd, s1, s2, mx, rows):
    """2^-k of the sp dy: k = 15 - exponent of the bound max |gamma invstd| (mx + |s1| / n + sqrt(n) |s2| / n) over (group,
    channel) (frexp: bound = m 2^e, m in [0.5, 1)).  Returns (2^-k, the bound's mantissa m: near 0.5 or 1 the fp32 evaluation
    of the bound may land on the other side of the power of two)."""
    n = float(rows)
    b = (gamma.double()[None] * invstd.double()).abs() * (mx.double() + s1.double().abs() / n + math.sqrt(n) * s2.double().abs() / n)
    m, e = math.frexp(float(b.max()))
    return 2.0 ** -(15 - e), m


# ---------------------------------------------------------------- case tables (expected query answers: 256 CUs)
# streaming passes: (name, elem, G, rows, C) -> accesses per group, grid.x, trips, step
STREAM_CASES = {
    ("two-trips", FP32, 1, 70000, 64): (1120000, 4096, 2, 0),
    ("two-trips", BF16, 1, 70000, 128): (1120000, 4096, 2, 0),
    ("two-trips", SP, 1, 70000, 128): (1120000, 4096, 2, 0),
    ("two-trips-step", FP32, 1, 48000, 96): (1152000, 4096, 2, 16),      # 2^20 mod 24 = 16
    ("two-trips-step", BF16, 1, 90000, 96): (1080000, 4096, 2, 4),       # 2^20 mod 12 = 4
    ("two-trips-step", SP, 1, 90000, 96): (1080000, 4096, 2, 4),
    ("groups", FP32, 3, 1000, 64): (16000, 63, 1, 0),
    ("groups", BF16, 3, 1000, 64): (8000, 32, 1, 0),
    ("groups", SP, 3, 1000, 64): (8000, 32, 1, 0),
}

# reduce-type passes over [rows][c]: (G, rows, C, CUs left (0: all 256)) -> per element kind (fp32 also: eval-bwd and the split
# reduce) cwn, cw, column blocks, row lanes, chunks, rows per chunk, empty chunks; None: rejected
REDUCE_CASES = {
    (1, 50000, 64, 0): {FP32: (16, 16, 1, 16, 768, 66, 10), BF16: (8, 8, 1, 32, 768, 66, 10)},        # the CU budget sets the chunks: ten get no rows
    (2, 64, 64, 0): {FP32: (16, 16, 1, 16, 1, 64, 0), BF16: (8, 8, 1, 32, 1, 64, 0)},                 # one chunk, exactly one unrolled trip
    (1, 37, 256, 0): {FP32: (64, 64, 1, 4, 1, 37, 0), BF16: (32, 32, 1, 8, 1, 37, 0)},                # one chunk: unrolled trips and a tail
    (1, 777, 1536, 0): {FP32: (384, 256, 2, 1, 13, 60, 0), BF16: None},                               # the last column block half masked
    (3, 1000, 2048, 0): {FP32: (512, 256, 2, 1, 16, 63, 0), BF16: (256, 256, 1, 1, 16, 63, 0)},
    (1, 5000, 64, 0): {FP32: (16, 16, 1, 16, 79, 64, 0), BF16: (8, 8, 1, 32, 79, 64, 0)},             # the 64-row floor ...
    (1, 5000, 64, 16): {FP32: (16, 16, 1, 16, 64, 79, 0), BF16: (8, 8, 1, 32, 64, 79, 0)},            # ... and 16 CUs' budget
}
REDUCE_REJECTED = "must divide 256 or be larger than 256"

# stem tail (pooled reduce / eval): (G, N, H, W, C, CUs left) -> (chunks, pooled lines per chunk) of the train-mode reduce,
# workgroups per group of the eval-mode pass
STEM_CASES = {
    (2, 3, 14, 18, 64, 0): ((11, 2), 12),         # ceil(756 / 64) = 12 chunks want ceil(21 / 12) = 2 lines each: 11 chunks
    (1, 2, 15, 13, 64, 0): ((6, 3), 7),           # ceil(390 / 64) = 7 chunks want ceil(16 / 7) = 3 lines each: 6 chunks
    (1, 1, 1, 7, 64, 0): ((1, 1), 1),
    (1, 2, 2, 2, 8, 0): ((1, 2), 1),
    (2, 9, 12, 12, 64, 8): ((18, 3), 16),         # 21 chunks want 3 of the 54 lines each: 18; eval: 21 workgroups of items, 4 x 8 / 2 allowed
    (1, 1, 4, 80, 8, 0): ((2, 1), 1),             # ceil(320 / 64) = 5 chunks, 2 pooled lines: clamped to one line each
}

# finalize: (G, partials, C, scratch registered) -> form, lanes per group, slices, partials per slice
FINALIZE_CASES = {
    (1, 40, 64, True): (WALK_GROUPS, 128, 0, 0),
    (1, 1100, 8, True): (WALK_GROUPS, 128, 62, 18),        # ceil(1100 / 64) = 18 per slice, ceil(1100 / 18) = 62 slices
    (2, 98, 20, True): (ALL_GROUPS, 64, 0, 0),
    (3, 130, 64, True): (ALL_GROUPS, 42, 0, 0),            # 3 x 42 lanes: lanes 126, 127 idle
    (4, 1219, 12, True): (ALL_GROUPS, 32, 61, 20),
    (5, 98, 20, True): (PER_GROUP, 128, 0, 0),
    (8, 1219, 8, True): (PER_GROUP, 128, 61, 20),
    (2, 98, 20, False): (ALL_GROUPS, 64, 0, 0),            # needs no scratch: the same form on a stream without any
    (3, 130, 64, False): (ALL_GROUPS, 42, 0, 0),
    (4, 1219, 12, False): (WALK_GROUPS, 128, 0, 0),        # no room for the slices: one workgroup walks the groups
    (5, 98, 20, False): (WALK_GROUPS, 128, 0, 0),
    (8, 1219, 8, False): (WALK_GROUPS, 128, 0, 0),
}
ROWS_PER_PARTIAL = 64


def finalize_rows(partials):
    """name -> (rows per group, partial slots): the row counts every finalize case runs."""
    rpp = ROWS_PER_PARTIAL
    return {"ragged": (partials * rpp - 17, partials), "exact": (partials * rpp, partials),
            "surplus": (max(partials - 5, 1) * rpp - 3, partials),        # valid < partials: NaN in the surplus slots
            "one-row": (1, partials), "one-over": (rpp + 1, partials)}


@functools.lru_cache(maxsize=None)
def finalize_data(G, partials, C, kind):
    """The fp32 rows [G, partials * 64, C] of a finalize case: `well` (O(1) mean and spread, per-channel offsets), `large-mean`
    (mean = 1e3 x the spread), `constant` (`well` with channels 0 .. 3 constant: variance 0)."""
    rows = partials * ROWS_PER_PARTIAL
    x = randn((G, rows, C), 1000 * G + partials + C) * (0.5 + torch.arange(C, dtype=torch.float32) / C)
    x = x + randn((G, 1, C), 7 * G + C)
    if kind == "large-mean":
        x = x + 1000.0 * (0.5 + torch.arange(C, dtype=torch.float32) / C)
    elif kind == "constant":
        for ch, v in enumerate((3.25, 0.1, -1234.567, 1e-3)):
            x[:, :, ch] = v
    else:
        assert kind == "well"
    return x.contiguous()


@functools.lru_cache(maxsize=None)
def finalize_params(C):
    """gamma, beta and non-trivial starting running statistics."""
    return (randn((C,), 11) * 0.3 + 1.0, randn((C,), 12) * 0.5, randn((C,), 13) * 0.7, torch.rand(C, generator=torch.Generator().manual_seed(14)) + 0.25)


@functools.lru_cache(maxsize=None)
def finalize_reference(G, partials, C, kind, rows_name, with_running=True):
    """(stats [G, slots, 2, C], rows, merge_partials(...)) of one finalize run; computed once, shared by the tests."""
    rows, slots = finalize_rows(partials)[rows_name]
    x = finalize_data(G, partials, C, kind)[:, :rows]
    stats = write_partials(x, ROWS_PER_PARTIAL, slots)
    gamma, beta, rm, rv = finalize_params(C)
    ref = merge_partials(stats, rows, ROWS_PER_PARTIAL, gamma, beta, rm if with_running else None, rv if with_running else None)
    return stats, rows, ref


def finalize_runs(G, partials):
    """(data kind, rows name, running statistics given) of every run of a finalize case: every row count on the well-conditioned
    set, the other sets and the null running statistics on the ragged one."""
    runs = [("well", r, True) for r in finalize_rows(partials)]
    return runs + [("large-mean", "ragged", True), ("constant", "ragged", True), ("well", "ragged", False)]
