"""The float64 reference of global-norm gradient clipping over arena segments: what mvg_grad_norm_segments must leave in its
device record, stated once for the CPU test (which pins it to torch.nn.utils.clip_grad_norm_) and the GPU tests.

    total  = sum of g^2 over the elements inside the segments, in float64
    norm   = sqrt(total)
    coef   = min(1, max_norm / (norm + 1e-6))          (torch's clip_coef_clamped; a NaN norm gives NaN, an infinite one 0)
             1 when max_norm is None or <= 0           (no clipping: the guard only)
    skipped = skip_nonfinite and total is not finite   (coef is then 0)

max_norm reaches the library as a C float, so the reference rounds it to float32 first.  ``record`` rounds norm and coef to
float32, which is what the device record holds."""
import math

import numpy as np
import torch


def sumsq(grad: torch.Tensor, bounds) -> float:
    """Sum of squares of grad over [(begin, end), ...] in float64 (a non-finite element makes it non-finite)."""
    g = grad.detach().to("cpu", torch.float64)
    return float(sum(float((g[b:e] * g[b:e]).sum().item()) for b, e, *_ in bounds))


def reference(grad: torch.Tensor, bounds, max_norm, skip_nonfinite: bool) -> dict:
    """{"norm", "coef", "skipped"} in float64 / bool."""
    total = sumsq(grad, bounds)
    norm = math.sqrt(total) if total == total and total >= 0 else float("nan")
    if max_norm is None or not float(max_norm) > 0:
        coef = 1.0
    else:
        c = float(np.float32(max_norm)) / (norm + 1e-6)
        coef = c if c != c else min(1.0, c)
    skipped = bool(skip_nonfinite) and not math.isfinite(total)
    return {"norm": norm, "coef": 0.0 if skipped else coef, "skipped": skipped}


def record(ref: dict):
    """(norm, coef) of ``reference`` rounded to float32, as numpy scalars."""
    with np.errstate(over="ignore"):
        return np.float32(ref["norm"]), np.float32(ref["coef"])


def within_one_ulp(got: float, want) -> bool:
    """got (a float32 value) is `want` (np.float32) or one of its two float32 neighbours; NaN matches NaN, inf matches inf."""
    got, want = np.float32(got), np.float32(want)
    if np.isnan(want) or np.isnan(got):
        return bool(np.isnan(want) and np.isnan(got))
    return bool(got == want or got == np.nextafter(want, np.float32(np.inf)) or got == np.nextafter(want, np.float32(-np.inf)))
