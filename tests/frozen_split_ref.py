"""NumPy restatement (float64) of the activation bound of a frozen-BatchNorm unit on the split kernels (csrc/bn.hip:
bn_frozen_finalize_kernel; include/rotmvgaze.h: mvg_bn_frozen_finalize), of the conv epilogue's statistics partials it reads, and
of the power-of-two rule that turns a bound into the scale of an sp tensor (elem.h: sp_scale_for_banded).

For one group g and channel c, with mean_b and the biased variance var_b of the n conv outputs y, every element obeys
|y - mean_b| <= sqrt((n - 1) var_b) (one deviation cannot exceed the root of the sum of all squared deviations, and the others'
sum to at least its square / (n - 1)).  Hence
    |gamma invstd_r (y - rm) + beta| <= |gamma| invstd_r (|mean_b - rm| + sqrt((n - 1) var_b)) + |beta|
    bound(unit) = max over (g, c);   bound(block output) = bound(last unit) + bound(identity)   (ReLU / max pool raise nothing)."""
import math

import numpy as np

MARGIN = 1.0 + 2.0 ** -7          # ops.FROZEN_BOUND_MARGIN: the kernel's final factor
TARGET_BITS = 15                  # a scaled bound lies in [2^14, 2^15): a factor of two below fp16's 65 520


def invstd_running(rv, eps):
    return 1.0 / np.sqrt(np.asarray(rv, np.float64) + eps)


def unit_bound_per_channel(y, gamma, beta, rm, rv, eps):
    """y [G, rows, c] -> the right-hand side above per (g, c), float64, no margin."""
    y = np.asarray(y, np.float64)
    n = y.shape[1]
    mean_b, var_b = y.mean(1), y.var(1)
    ga, be, rm = (np.asarray(t, np.float64) for t in (gamma, beta, rm))
    return np.abs(ga) * invstd_running(rv, eps) * (np.abs(mean_b - rm) + np.sqrt((n - 1) * var_b)) + np.abs(be)


def unit_bound(y, gamma, beta, rm, rv, eps):
    return float(unit_bound_per_channel(y, gamma, beta, rm, rv, eps).max())


def normalised(y, gamma, beta, rm, rv, eps):
    """The unit's BatchNorm output on the running statistics, float64."""
    y = np.asarray(y, np.float64)
    ga, be, rm = (np.asarray(t, np.float64) for t in (gamma, beta, rm))
    return ga * invstd_running(rv, eps) * (y - rm) + be


def scale_for(bound):
    """2^k of an sp activation with this bound: 1 while 1 <= bound < 2^15, else the power of two that maps the bound into
    [2^14, 2^15); a zero, negative, infinite or NaN bound gives 1."""
    b = float(bound)
    if 1.0 <= b < 2.0 ** TARGET_BITS:
        return 1.0
    if not (b > 0.0) or not (b < 3.0e38):
        return 1.0
    _, e = math.frexp(b)              # b = m 2^e, m in [0.5, 1)
    k = max(-100, min(100, TARGET_BITS - e))
    return math.ldexp(1.0, k)


def sinv_for(bound):
    return 1.0 / scale_for(bound)


def partials(y32, rows_per_partial, n_partials=None):
    """The conv epilogue's record of y32 [G, rows, c] (fp32 values): [G, P, 2, c] fp32 - per row tile the sum and the sum of
    squared deviations from the tile's own mean (the layout mvg_bn_finalize reads).  The last tile may be ragged; tiles past
    the rows (n_partials > the tiles needed) stay NaN: nobody may read them."""
    y = np.asarray(y32, np.float32).astype(np.float64)
    G, rows, c = y.shape
    need = -(-rows // rows_per_partial)
    P = need if n_partials is None else n_partials
    assert P >= need
    out = np.full((G, P, 2, c), np.nan, np.float32)
    for p in range(need):
        t = y[:, p * rows_per_partial:(p + 1) * rows_per_partial]
        out[:, p, 0] = t.sum(1)
        out[:, p, 1] = ((t - t.mean(1, keepdims=True)) ** 2).sum(1)
    return out
