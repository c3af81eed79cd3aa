"""Test helper (not collected, not imported by the package): the per-tensor scales of the backbone's sp activations,
evaluated on the host from a state dict and the input shape alone, and the modified state dicts the range tests use.

    bound(unit)            = max over channels of (|gamma_c| * sqrt(n - 1) + |beta_c|),  n = B * Ho * Wo per view
    bound(block output)    = bound(last unit) + bound(identity)
    bound(identity)        = bound of the previous block's output, or bound(downsample BatchNorm) when the block has one
    bound(stem pooled map) = bound(stem unit)
    2^k = 1 while 1 <= bound < 2^15, else the power of two that maps the bound just below 2^15; zero / non-finite bound: 1

in fp32 with one rounding per operation, which is what the device evaluates (a plain multiply and a plain add per
channel, a maximum, one add per chain link): the slots must agree exactly."""
import functools
import math
from collections import OrderedDict

import numpy as np

from rot_mvgaze_amd import synth
from rot_mvgaze_amd.arch import backbone_spec

P = "_feat_extractor.0."


@functools.lru_cache(maxsize=None)
def _base_state_dict(depth, conditioned, perturb_bn):
    return OrderedDict((k, np.array(v)) for k, v in synth.make_state_dict(depth, 0, 3, perturb_bn=perturb_bn, conditioned=conditioned).items())


def modified_state_dict(depth, bn=None, factor=1.0, conditioned=False, perturb_bn=True):
    """The seeded recipe with gamma AND beta of BatchNorm `bn` (name without the prefix, e.g. "layer2.0.bn1") times factor.
    (The unmodified arrays are shared between calls: replace entries, do not write into them.)"""
    sd = OrderedDict(_base_state_dict(depth, conditioned, perturb_bn))
    if bn is not None:
        for leaf in (".weight", ".bias"):
            sd[P + bn + leaf] = (sd[P + bn + leaf] * np.float32(factor)).astype(np.float32)
    return sd


def unit_bound(gamma, beta, n):
    s = np.float32(math.sqrt(max(n - 1, 0)))
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.abs(gamma.astype(np.float32)) * s + np.abs(beta.astype(np.float32))
        v = np.where(v <= np.float32(3.0e38), v, np.float32(np.inf))          # NaN too
    return np.float32(v.max())


def sinv_for(bound):
    """2^-k for a bound (the banded rule)."""
    b = float(bound)
    if not (b > 0.0) or not (b < 3.0e38) or 1.0 <= b < 32768.0:
        return 1.0
    _, e = math.frexp(b)
    return 2.0 ** -max(-100, min(100, 15 - e))


def _size(h, c):
    return (h + 2 * c.pad - c.k) // c.stride + 1


def expected_bounds(sd, depth, B, H, W):
    """conv name -> bound of the sp tensor that unit writes (the stem: its pooled map), in forward order."""
    spec = backbone_spec(depth)

    def ub(c, n):
        return unit_bound(np.asarray(sd[c.bn + ".weight"]), np.asarray(sd[c.bn + ".bias"]), n)
    out = OrderedDict()
    h, w = _size(H, spec.stem), _size(W, spec.stem)
    prev = out[spec.stem.name] = ub(spec.stem, B * h * w)
    h, w = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
    for blk in spec.blocks:
        hb, wb = h, w
        for c in blk.convs[:-1]:
            hb, wb = _size(hb, c), _size(wb, c)
            out[c.name] = ub(c, B * hb * wb)
        ident = prev
        if blk.downsample is not None:
            ident = ub(blk.downsample, B * _size(h, blk.downsample) * _size(w, blk.downsample))
        c = blk.convs[-1]
        hb, wb = _size(hb, c), _size(wb, c)
        with np.errstate(invalid="ignore", over="ignore"):
            prev = out[c.name] = np.float32(ub(c, B * hb * wb) + ident)
        h, w = hb, wb
    return out


def expected_sinv(sd, depth, B, H, W):
    return OrderedDict((k, sinv_for(v)) for k, v in expected_bounds(sd, depth, B, H, W).items())


# (depth, batch, px, conditioned, BatchNorm, factor): gamma and beta of ONE BatchNorm times a power of two, so that the fp32
# arithmetic around the tensor is exactly scale-equivariant and only its storage can differ
RANGE_CASES = [
    (18, 8, 64, False, "layer2.0.bn1", 2.0 ** 16),              # a plain unit
    (18, 8, 64, False, "bn1", 2.0 ** 16),                       # the stem: the pooled map
    (18, 8, 64, False, "layer1.1.bn2", 2.0 ** 16),              # a block's last unit: the block output
    (18, 8, 64, False, "bn1", 2.0 ** -14),                      # small activations: accuracy, not overflow
    (50, 4, 64, True, "layer2.0.bn2", 2.0 ** 16),               # a plain unit
    (50, 4, 64, True, "bn1", 2.0 ** 16),
    (50, 4, 64, True, "layer1.0.downsample.1", 2.0 ** 16),      # a downsample BatchNorm: the identity of a block output
    (50, 4, 64, True, "layer1.0.bn3", 2.0 ** 20),               # a block's last unit (its gamma is x 0.1 in this recipe)
    (50, 4, 64, True, "layer3.2.bn3", 2.0 ** 20),
    (50, 4, 64, True, "bn1", 2.0 ** -14),
]
RANGE_IDS = ["r%d_b%d_hw%d_%s_2^%+d" % (d, b, hw, bn, round(math.log2(f))) for d, b, hw, _c, bn, f in RANGE_CASES]
