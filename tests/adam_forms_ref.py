"""The float64 reference of ONE Adam step (torch.optim.Adam: coupled L2 weight decay, bias correction, no amsgrad) on flat arrays,
its per-element error units, and the case table of tests/test_adam_forms_gpu.py (checked without a GPU in
tests/test_adam_forms_cpu.py).  Every Adam entry point of csrc/adam.hip (adam_elem / adam_slot / adam_tick1) is held to this one statement.

    lr, b1, b2, eps, wd, coef   rounded to float32 first: the values the C ABI carries
    g      = float32(g * coef) for the clipped forms, rounded on its own (clip_mul)
    g_r    = g + wd * p
    m'     = b1 * m + (1 - b1) * g_r
    v'     = b2 * v + (1 - b2) * g_r^2
    bc1    = 1 - b1^step, bc2 = 1 - b2^step              in float64, from the float32 betas
    s      = sqrt(v') / sqrt(bc2),  den = s + eps
    d      = (lr / bc1) * m' / den,  p' = p - d
    state_row(step, b1, b2) = {step, bc1, sqrt(bc2)}     what a device row holds after the tick that reaches `step`
    a skipped step (clip4[2] != 0) changes nothing and advances no row

Units.  First-order running error bounds, carried with the values, so that a comparison is neither fooled by cancellation
(b1 * m against (1 - b1) * g_r) nor hidden behind |p|:
    U_g = |g| + |wd * p|
    U_m = |b1 * m| + (1 - b1) * U_g
    U_v = v' + 2 (1 - b2) |g_r| U_g
    U_d = |d| + (lr / bc1) / den * (U_m + |m'| (s / den) U_v / (2 v'))          (the last term is 0 where v' = 0)
    U_p = |p'| + U_d
An element passes when |got - want| <= K * 2^-24 * U for each of m, v and p.

K_M, K_V, K_P are four times the worst figure of `float32_restatement` (the same operation order in NumPy float32, no fused
multiply-add) over every problem of the table (`measured_problems`), rounded up to an integer; tests/test_adam_forms_cpu.py
measures them and asserts that the constants below are those.  The margin of four is IBN_SCALES_BAR's
(tests/fusion_kernels_ref.py): it covers the contraction into fused multiply-adds and the operation order the kernel is free to
choose.  The GPU test imports the constants; nothing is re-fitted to the kernel.  Measured here (worst units of the restatement
over the table, the two BIG_N problems included): m 2.893, v 1.989, p 1.793."""
import math

import numpy as np

EPS24 = 2.0 ** -24

K_M, K_V, K_P = 12, 8, 8

# (lr, beta1, beta2, eps, weight decay, step): the Python doubles a user passes
HYPER = [
    (1e-3, 0.9, 0.999, 1e-8, 1e-6, 1),
    (1e-3, 0.9, 0.999, 1e-8, 1e-2, 3),
    (5e-2, 0.5, 0.9, 1e-3, 0.1, 100),
    (1e-4, 0.3, 0.99, 1e-6, 0.0, 7),
    (1e-3, 0.0, 0.9999, 1e-8, 1e-6, 100000),
    (1e-2, 0.95, 0.999, 1e-5, 1e-3, 1000),
]
SCALES = (1.0, 1e-4, 0.0)
SIZES = (4, 8, 1020, 4100)
BIG_N = 8192 * 256 * 4 + 512                      # past the flat update kernels' grid cap: the grid-stride loop's second pass
BIG = {"adam_step": (1, 0), "adam_step_dev": (5, 1)}          # entry -> (hyper, scale index) of its one BIG_N case


def f32(x) -> float:
    return float(np.float32(x))


def hyper32(h):
    """(lr, b1, b2, eps, wd) of HYPER[h] as the C ABI's floats carry them, and the step."""
    lr, b1, b2, eps, wd, step = HYPER[h]
    return f32(lr), f32(b1), f32(b2), f32(eps), f32(wd), int(step)


def state_row(step, b1, b2):
    """{step, 1 - b1^step, sqrt(1 - b2^step)} in float64 from the float32 betas."""
    b1, b2 = f32(b1), f32(b2)
    return np.array([float(step), 1.0 - b1 ** float(step), math.sqrt(1.0 - b2 ** float(step))], dtype=np.float64)


def reference(p, g, m, v, lr, b1, b2, eps, wd, step, coef=None, skipped=False, mutation=None):
    """One step in float64 with its units: {"p", "m", "v", "d", "U_p", "U_m", "U_v", "U_d", "g_r"}.  ``mutation`` (the CPU test's
    sensitivity check only) states one wrong Adam; the units are always those of the right one's formulas on the values computed."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    b2_user = float(b2)
    lr, b1, b2, eps, wd = f32(lr), f32(b1), f32(b2), f32(eps), f32(wd)
    if coef is not None:
        g = (g * f32(coef)).astype(np.float32).astype(np.float64)
    if skipped:
        z = np.zeros_like(p)
        return {"p": p.copy(), "m": m.copy(), "v": v.copy(), "d": z, "U_p": np.abs(p), "U_m": np.abs(m), "U_v": np.abs(v), "U_d": z,
                "g_r": z}
    if mutation == "lanes_xy_swapped":
        g = g.copy().reshape(-1, 4)
        g[:, [0, 1]] = g[:, [1, 0]]
        g = g.reshape(-1)
    g_r = g if mutation == "decoupled_weight_decay" else g + wd * p
    g_v = g if mutation == "v_from_g" else g_r
    m2 = b1 * m + (1.0 - b1) * g_r
    v2 = b2 * v + (1.0 - b2) * g_v * g_v
    bc1 = 1.0 if mutation == "bc1_omitted" else 1.0 - b1 ** float(step)
    bc2 = 1.0 - (b2_user if mutation == "bc2_from_double_beta" else b2) ** float(step)
    if mutation == "eps_inside_bc2_division":
        den = (np.sqrt(v2) + eps) / math.sqrt(bc2)
        s = den - eps
    else:
        s = np.sqrt(v2) / math.sqrt(bc2)
        den = s + eps
    d = (lr / bc1) * m2 / den
    p2 = p - d
    if mutation == "decoupled_weight_decay":
        p2 = p2 - lr * wd * p
        d = p - p2
    U_g = np.abs(g) + np.abs(wd * p)
    U_m = np.abs(b1 * m) + (1.0 - b1) * U_g
    U_v = v2 + 2.0 * (1.0 - b2) * np.abs(g_r) * U_g
    with np.errstate(divide="ignore", invalid="ignore"):
        tail = np.where(v2 > 0, np.abs(m2) * (s / den) * U_v / (2.0 * v2), 0.0)
    U_d = np.abs(d) + (lr / bc1) / den * (U_m + tail)
    return {"p": p2, "m": m2, "v": v2, "d": d, "U_p": np.abs(p2) + U_d, "U_m": U_m, "U_v": U_v, "U_d": U_d, "g_r": g_r}


MUTATIONS = ("decoupled_weight_decay", "eps_inside_bc2_division", "bc2_from_double_beta", "bc1_omitted", "v_from_g", "lanes_xy_swapped")


def float32_restatement(p, g, m, v, lr, b1, b2, eps, wd, step, coef=None):
    """adam_elem's coupled branch as csrc/adam.hip writes it, every operation rounded to float32 on its own (NumPy: no fused multiply-add); the bias
    corrections from double pow rounded to float32 as the launchers and adam_tick1 form them.  For tests/test_adam_forms_cpu.py."""
    F = np.float32
    p, g, m, v = (np.asarray(a, dtype=F) for a in (p, g, m, v))
    lr, b1, b2, eps, wd = F(lr), F(b1), F(b2), F(eps), F(wd)
    if coef is not None:
        g = g * F(coef)
    bc1 = F(1.0 - float(b1) ** float(step))
    bc2_sqrt = F(math.sqrt(1.0 - float(b2) ** float(step)))
    step_size = lr / bc1
    gr = g + wd * p
    m2 = b1 * m + (F(1) - b1) * gr
    v2 = b2 * v + (F(1) - b2) * gr * gr
    den = np.sqrt(v2) / bc2_sqrt + eps
    p2 = p - step_size * (m2 / den)
    assert p2.dtype == m2.dtype == v2.dtype == F
    return p2, m2, v2


def units(got, want, U):
    """|got - want| / (2^-24 U) per element; 0 where both agree exactly, inf where they differ and the unit is 0."""
    diff = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = diff / (EPS24 * U)
    return np.where(diff == 0, 0.0, np.where(U > 0, u, np.inf))


def worst_units(ref, got_p, got_m, got_v):
    """(m, v, p) worst units of one problem (NaN if an output is not finite)."""
    out = []
    for got, key in ((got_m, "m"), (got_v, "v"), (got_p, "p")):
        got = np.asarray(got, dtype=np.float64)
        out.append(float(units(got, ref[key], ref["U_" + key]).max()) if np.isfinite(got).all() else float("nan"))
    return tuple(out)


def step_max_rel(ref, p_before, got_p):
    """max |d_got - d_ref| / max |d_ref| (the figure the parameter-relative bars never bounded); 0 when no element moves."""
    d = np.asarray(p_before, dtype=np.float64) - np.asarray(got_p, dtype=np.float64)
    top = float(np.abs(ref["d"]).max())
    return float(np.abs(d - ref["d"]).max()) / top if top > 0 else float(np.abs(d).max())


# ---------------------------------------------------------------- the inputs
def inputs(n, scale, step, seed):
    """p = scale * randn, |g| log-uniform in 1e-6 .. 1 with a random sign, m ~ 0.01 randn, v ~ 1e-3 rand (m = v = 0 at step 1)."""
    rng = np.random.default_rng(seed)
    p = (scale * rng.standard_normal(n)).astype(np.float32)
    g = (10.0 ** rng.uniform(-6.0, 0.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    m = (0.01 * rng.standard_normal(n)).astype(np.float32)
    v = (1e-3 * rng.random(n)).astype(np.float32)
    if step == 1:
        m[:] = 0
        v[:] = 0
    return p, g, m, v


def nan_pattern(n, salt):
    """n distinct quiet-NaN bit patterns (payload = position and salt): what the holes of an arena hold."""
    bits = (0x7FC00000 + 1 + ((np.arange(n, dtype=np.int64) * 4 + salt) & 0x3FFFFF)).astype(np.uint32)
    return bits.view(np.float32)


class Arena:
    """One problem: arrays p, g, m, v of n floats, segments [(begin, end, hyper index)] filled by `inputs` (each segment with its
    own seed and its hyper set's step), NaN patterns everywhere else."""

    def __init__(self, name, n, segs, scale, seed):
        self.name, self.n, self.segs, self.scale = name, n, segs, scale
        self.p, self.g, self.m, self.v = (nan_pattern(n, salt).copy() for salt in range(4))
        for k, (b, e, h) in enumerate(segs):
            for dst, src in zip((self.p, self.g, self.m, self.v), inputs(e - b, scale, HYPER[h][5], seed * 1000 + k)):
                dst[b:e] = src

    def outside(self):
        mask = np.ones(self.n, dtype=bool)
        for b, e, _ in self.segs:
            mask[b:e] = False
        return mask

    def grad_sumsq(self):
        return float(sum(float((self.g[b:e].astype(np.float64) ** 2).sum()) for b, e, _ in self.segs))

    def clip(self, fraction=0.37):
        """(max_norm, coef) in float32 for a max_norm of `fraction` of the segments' gradient norm (grad_clip_ref's rule)."""
        norm = math.sqrt(self.grad_sumsq())
        max_norm = f32(fraction * norm)
        return max_norm, f32(min(1.0, max_norm / (norm + 1e-6)))

    def references(self, coef=None, skipped=False, state=None, lrs=None):
        """One `reference` per segment.  state: (p, m, v) to start from instead of the arena's own; lrs: per-segment learning rate
        and step = [(lr, step)] instead of the table's (the teacher-forced sequences)."""
        p, m, v = (self.p, self.m, self.v) if state is None else state
        out = []
        for k, (b, e, h) in enumerate(self.segs):
            lr, b1, b2, eps, wd, step = HYPER[h]
            if lrs is not None:
                lr, step = lrs[k]
            out.append(reference(p[b:e], self.g[b:e], m[b:e], v[b:e], lr, b1, b2, eps, wd, step, coef=coef, skipped=skipped))
        return out

    def compare(self, refs, got_p, got_m, got_v, p_before=None):
        """Worst (m, v, p) units and step max-rel over the segments."""
        p_before = self.p if p_before is None else p_before
        worst, rel = [0.0, 0.0, 0.0], 0.0
        for (b, e, _), r in zip(self.segs, refs):
            w = worst_units(r, got_p[b:e], got_m[b:e], got_v[b:e])
            worst = [x if (x != x or x >= y) else y for x, y in zip(w, worst)]
            rel = max(rel, step_max_rel(r, p_before[b:e], got_p[b:e]))
        return tuple(worst), rel


def flat_arenas():
    """n = 4100 at every hyper set x scale, n = 4, 8, 1020 at every hyper set with the scale rotating: 36 one-segment problems."""
    out = []
    for h in range(len(HYPER)):
        for si, scale in enumerate(SCALES):
            out.append(Arena(f"h{h}_scale{scale:g}_n4100", 4100, [(0, 4100, h)], scale, seed=100 + 10 * h + si))
    for ni, n in enumerate(SIZES[:3]):
        for h in range(len(HYPER)):
            scale = SCALES[(h + ni) % 3]
            out.append(Arena(f"h{h}_scale{scale:g}_n{n}", n, [(0, n, h)], scale, seed=300 + 10 * h + ni))
    return out


def big_arena(entry):
    h, si = BIG[entry]
    return Arena(f"h{h}_scale{SCALES[si]:g}_n{BIG_N}", BIG_N, [(0, BIG_N, h)], SCALES[si], seed=900 + h)


def three_segments(lengths, n):
    """A 4-element segment at 0, one behind a hole, one ending at n."""
    a, b, c = lengths
    assert a == 4 and 64 + b < n - c
    return [(0, 4), (64, 64 + b), (n - c, n)]


THREE_LAYOUTS = {"three_4_1020_4100": ((4, 1020, 4100), 5244), "three_4_8_1020": ((4, 8, 1020), 1148)}


def thirty_five_bounds(seed=3):
    """35 segments (16 + 16 + 3: three launches) of 4 .. 64 elements with holes of 0 .. 16 elements (the
    recipe of tests/test_adam_segments_dev_gpu.py)."""
    rng = np.random.default_rng(seed)
    bounds, off = [], 0
    for _ in range(35):
        off += 4 * int(rng.integers(0, 5))
        ln = 4 * int(rng.integers(1, 17))
        bounds.append((off, off + ln))
        off += ln
    return bounds, off + 64


def segment_arenas():
    """The segmented entry points' problems: both three-segment layouts at six rotations of the hyper sets (segment k of rotation
    r takes set (r + k) % 6), the scale rotating, and the 35-segment layout at the three scales (segment i takes set i % 6)."""
    out = []
    for li, (name, (lengths, n)) in enumerate(sorted(THREE_LAYOUTS.items())):
        for r in range(len(HYPER)):
            scale = SCALES[(r + li) % 3]
            segs = [(b, e, (r + k) % len(HYPER)) for k, (b, e) in enumerate(three_segments(lengths, n))]
            out.append(Arena(f"{name}_rot{r}_scale{scale:g}", n, segs, scale, seed=500 + 10 * r + li))
    bounds, n = thirty_five_bounds()
    for si, scale in enumerate(SCALES):
        segs = [(b, e, (i + si) % len(HYPER)) for i, (b, e) in enumerate(bounds)]
        out.append(Arena(f"thirty_five_scale{scale:g}", n, segs, scale, seed=700 + si))
    return out


def sequence_arena():
    """n = 4100 for the teacher-forced sequence of the segmented device form: [0, 4), [16, 1036), [1100, 4100), zero moments."""
    a = Arena("sequence_n4100", 4100, [(0, 4, 3), (16, 1036, 1), (1100, 4100, 2)], 1.0, seed=800)
    for b, e, _ in a.segs:
        a.m[b:e] = 0
        a.v[b:e] = 0
    return a


def sequence_gradient(n, step, seed=810):
    """The fresh gradient of step `step` of a sequence (the recipe's |g|)."""
    return inputs(n, 1.0, 2, 100 * seed + step)[1]


def sequence_lr(lr, step):
    """The learning rate of step `step` (1-based) of a sequence: a triangular walk between 0.2 and 1 times lr, as float32."""
    return f32(lr * (0.2 + 0.8 * abs(((step * 3) % 10) - 5) / 5.0))


# the device forms' learning-rate table: six slots in reverse order of the hyper sets between two that no segment may read
def lr_table():
    return [float("nan")] + [f32(HYPER[h][0]) for h in reversed(range(len(HYPER)))] + [float("nan")]


def lr_index(h):
    return len(HYPER) - h


def problems():
    """Every (name, arena, coef) the GPU test holds to the bars: what K is measured over.  The clipped forms run the segment
    arenas with the coefficient of `Arena.clip` and with coef = 1; the unclipped ones with none (equal to coef = 1 in every bit)."""
    for a in flat_arenas():
        yield a.name, a, None
    for a in segment_arenas():
        yield a.name, a, None
        yield a.name + "_clipped", a, a.clip()[1]


def measured_problems():
    """`problems` and the two BIG_N cases: everything K_M, K_V, K_P are measured over."""
    yield from problems()
    for entry in sorted(BIG):
        a = big_arena(entry)
        yield a.name, a, None
