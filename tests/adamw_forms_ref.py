"""The float64 reference of ONE Adam step with DECOUPLED weight decay (torch.optim.AdamW; no amsgrad) on flat arrays, its per-element
error units and the bars of tests/test_adamw_forms_gpu.py and tests/test_adamw_optim_gpu.py (checked without a GPU in
tests/test_adamw_forms_cpu.py).  The case table, the inputs, `Arena`, `units` and the coupled reference are adam_forms_ref's,
imported and never copied; every decoupled entry point of csrc/adam.hip (adam_elem<true> / adam_slot / adamw_factor) is held to this one
statement.

    lr, b1, b2, eps, wd, coef   rounded to float32 first: the values the C ABI carries
    g      = float32(g * coef) for the clipped forms, rounded on its own (clip_mul)
    f      = 1 - lr * wd                                 lr the plain learning rate, not lr / bc1
    q      = p * f
    m'     = b1 * m + (1 - b1) * g                       the gradient alone: no wd * p in the moments
    v'     = b2 * v + (1 - b2) * g^2
    bc1    = 1 - b1^step, bc2 = 1 - b2^step              in float64, from the float32 betas
    s      = sqrt(v') / sqrt(bc2),  den = s + eps
    d      = (lr / bc1) * m' / den,  p' = q - d
    a skipped step (clip4[2] != 0) changes nothing and advances no row

Units (adam_forms_ref's, with the decay moved from the gradient to the parameter):
    U_g = |g|
    U_m = |b1 * m| + (1 - b1) * U_g
    U_v = v' + 2 (1 - b2) |g| U_g
    U_d = |d| + (lr / bc1) / den * (U_m + |m'| (s / den) U_v / (2 v'))          (the last term is 0 where v' = 0)
    U_p = |p'| + |q| + |lr * wd * p| + U_d
An element passes when |got - want| <= K * 2^-24 * U for each of m, v and p.  |q| stands for the rounding of the product p * f,
|lr * wd * p| for the two roundings inside f (lr * wd and 1 - lr * wd, the latter one half ulp of ~1 times |p|, which the
term |q| also covers).

K_M, K_V, K_P follow adam_forms_ref's rule: four times the worst figure of `float32_restatement` (the kernel's operation order in
NumPy float32, no fused multiply-add) over every problem of the table (`adam_forms_ref.measured_problems`, the two BIG_N problems
included, every segment decoupled), rounded up to an integer; tests/test_adamw_forms_cpu.py measures them and asserts that the
constants below are those.  The GPU tests import the constants; nothing is re-fitted to the kernel.  Measured here (worst units
of the restatement over the table): m 1.986, v 1.986, p 1.712, all three on the BIG_N problem of hyper set 5 (over the flat and
segment arenas alone: m 1.920, v 1.913, p 1.313)."""
import math

import numpy as np

import adam_forms_ref as R
from adam_forms_ref import HYPER, f32

K_M, K_V, K_P = 8, 8, 7

MUTATIONS = ("f_from_step_size", "f_plus", "lanes_xy_swapped")


def reference(p, g, m, v, lr, b1, b2, eps, wd, step, coef=None, skipped=False, mutation=None):
    """One decoupled step in float64 with its units: the keys of adam_forms_ref.reference ("g_r" is the gradient the moments saw)
    and "q".  ``mutation`` (the CPU test's sensitivity check only) states one wrong AdamW: f = 1 - (lr / bc1) * wd
    ("f_from_step_size"), f = 1 + lr * wd ("f_plus") or the x and y lanes of the gradient swapped ("lanes_xy_swapped")."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    lr, b1, b2, eps, wd = f32(lr), f32(b1), f32(b2), f32(eps), f32(wd)
    if coef is not None:
        g = (g * f32(coef)).astype(np.float32).astype(np.float64)
    if skipped:
        z = np.zeros_like(p)
        return {"p": p.copy(), "m": m.copy(), "v": v.copy(), "d": z, "U_p": np.abs(p), "U_m": np.abs(m), "U_v": np.abs(v), "U_d": z,
                "g_r": z, "q": p.copy()}
    if mutation == "lanes_xy_swapped":
        g = g.copy().reshape(-1, 4)
        g[:, [0, 1]] = g[:, [1, 0]]
        g = g.reshape(-1)
    bc1 = 1.0 - b1 ** float(step)
    bc2 = 1.0 - b2 ** float(step)
    f = 1.0 - lr * wd
    if mutation == "f_from_step_size":
        f = 1.0 - (lr / bc1) * wd
    elif mutation == "f_plus":
        f = 1.0 + lr * wd
    q = p * f
    m2 = b1 * m + (1.0 - b1) * g
    v2 = b2 * v + (1.0 - b2) * g * g
    s = np.sqrt(v2) / math.sqrt(bc2)
    den = s + eps
    d = (lr / bc1) * m2 / den
    p2 = q - d
    U_g = np.abs(g)
    U_m = np.abs(b1 * m) + (1.0 - b1) * U_g
    U_v = v2 + 2.0 * (1.0 - b2) * np.abs(g) * U_g
    with np.errstate(divide="ignore", invalid="ignore"):
        tail = np.where(v2 > 0, np.abs(m2) * (s / den) * U_v / (2.0 * v2), 0.0)
    U_d = np.abs(d) + (lr / bc1) / den * (U_m + tail)
    U_p = np.abs(p2) + np.abs(q) + np.abs(lr * wd * p) + U_d
    return {"p": p2, "m": m2, "v": v2, "d": d, "U_p": U_p, "U_m": U_m, "U_v": U_v, "U_d": U_d, "g_r": g, "q": q}


def float32_restatement(p, g, m, v, lr, b1, b2, eps, wd, step, coef=None):
    """adam_elem's decoupled branch as csrc/adam.hip writes it, every operation rounded to float32 on its own (NumPy: no fused multiply-add); the bias
    corrections from double pow rounded to float32 as the launchers and adam_tick1 form them.  For tests/test_adamw_forms_cpu.py."""
    F = np.float32
    p, g, m, v = (np.asarray(a, dtype=F) for a in (p, g, m, v))
    lr, b1, b2, eps, wd = F(lr), F(b1), F(b2), F(eps), F(wd)
    if coef is not None:
        g = g * F(coef)
    bc1 = F(1.0 - float(b1) ** float(step))
    bc2_sqrt = F(math.sqrt(1.0 - float(b2) ** float(step)))
    step_size = lr / bc1
    f = F(1) - lr * wd
    q = p * f
    m2 = b1 * m + (F(1) - b1) * g
    v2 = b2 * v + (F(1) - b2) * g * g
    den = np.sqrt(v2) / bc2_sqrt + eps
    p2 = q - step_size * (m2 / den)
    assert p2.dtype == m2.dtype == v2.dtype == F and type(f) is F
    return p2, m2, v2


def step_max_rel(ref, p_before, got_p):
    """adam_forms_ref.step_max_rel for either mode: max |move_got - move_ref| / max |move_ref| with move = p - p', the decay's
    share included (a decoupled reference's "d" is the Adam step alone); 0 when no element moves."""
    p_before = np.asarray(p_before, dtype=np.float64)
    move = p_before - ref["p"]
    err = float(np.abs((p_before - np.asarray(got_p, dtype=np.float64)) - move).max())
    top = float(np.abs(move).max())
    return err / top if top > 0 else err


def references(arena, coef=None, skipped=False, state=None, lrs=None, modes=None):
    """`Arena.references` with a mode per segment: one `reference` (mode 1, the default for every segment) or
    `adam_forms_ref.reference` (mode 0) per segment of ``arena``; state, lrs as there."""
    p, m, v = (arena.p, arena.m, arena.v) if state is None else state
    out = []
    for k, (b, e, h) in enumerate(arena.segs):
        lr, b1, b2, eps, wd, step = HYPER[h]
        if lrs is not None:
            lr, step = lrs[k]
        ref = reference if modes is None or modes[k] else R.reference
        out.append(ref(p[b:e], arena.g[b:e], m[b:e], v[b:e], lr, b1, b2, eps, wd, step, coef=coef, skipped=skipped))
    return out


def slice_arena(arena, k):
    """Segment k of ``arena`` as a one-segment arena of its own (the same values): what the plain entry points run over when a
    segmented result is compared with theirs bit for bit."""
    b, e, h = arena.segs[k]
    a = R.Arena(f"{arena.name}_seg{k}", e - b, [(0, e - b, h)], arena.scale, seed=0)
    a.p[:], a.g[:], a.m[:], a.v[:] = arena.p[b:e], arena.g[b:e], arena.m[b:e], arena.v[b:e]
    return a
