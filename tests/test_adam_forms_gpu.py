"""Every Adam entry point of csrc/adam.hip called directly (ops.*) and held, element by element, to the float64 statement of one
torch.optim.Adam step in tests/adam_forms_ref.py - the parameter, both moments and, for the device forms, the state rows their tick
kernels advance.  Runs on an MI355X only; the reference, its units, the bars and the case table are checked without a GPU in
tests/test_adam_forms_cpu.py.

An element passes when |got - want| <= K * 2^-24 * U with the propagated units U_m, U_v, U_p of the reference and K_M = 12,
K_V = 8, K_P = 8: four times what the same operation order costs in NumPy float32, measured on the CPU over this very table and
never re-fitted to the kernel.  Every comparison prints
    ADAM-FORMS <entry> <case>: m <units> v <units> p <units>   step max-rel <max |d_got - d_ref| / max |d_ref|>
before it asserts the outputs finite and inside the bars; the device forms add a line for their tick kernel (state rows within one
float32 ulp of {step, 1 - b1^step, sqrt(1 - b2^step)}).  Holes of the segmented arenas hold distinct NaN patterns in p, g, m and v and
must come back bit for bit; a skipped step must leave everything bit for bit, the rows included.

Cases (adam_forms_ref): six hyper sets x p-scales 1 / 1e-4 / 0 at n = 4100 and n = 4, 8, 1020 for the two plain entry points, which
also take n = 8192 * 256 * 4 + 512 once each (their own grid-stride loop); for the four segmented ones two three-segment layouts
with holes (4 + 1020 + 4100 and 4 + 8 + 1020 elements, each segment its own hyper set, six rotations) and 35 segments in three
launches; the clipped forms on a record mvg_grad_norm_segments wrote (coef 0.37) and on a hand-written coef = 1.  Twenty
teacher-forced steps of mvg_adam_step and mvg_adam_step_segments_dev walk step, both bias corrections and the tick through 1 .. 20
with a learning rate that changes every step, each step held to the reference evaluated from the kernel's own previous state.

Measured on an MI355X (every line: profiles/adam_forms_errors.txt), smallest .. largest units over the cases, next to K:
  entry point (kernel)                                   m            K_M   v            K_V   p            K_P   step max-rel
  mvg_adam_step                (36 cases, nan lanes)     0 .. 1.969   12    0.58 .. 1.979   8   0.27 .. 1.466   8   1.5e-08 .. 4.8e-04
  mvg_adam_step                n = 8192 * 256 * 4 + 512  1.935        12    1.979           8   1.466           8   6.4e-06
  mvg_adam_step_dev            (36 cases)                0 .. 1.985   12    0.58 .. 1.988   8   0.27 .. 1.708   8   1.5e-08 .. 4.8e-04
  mvg_adam_step_dev            n = 8192 * 256 * 4 + 512  1.985        12    1.988           8   1.708           8   7.2e-08
  mvg_adam_step_segments       (15 layouts)              1.03 .. 1.832  12  0.79 .. 1.886   8   0.92 .. 1.342   8   1.1e-07 .. 1.4e-03
  mvg_adam_step_segments_dev   (15 layouts)              1.03 .. 1.832  12  0.79 .. 1.886   8   0.92 .. 1.342   8   1.1e-07 .. 1.4e-03
  mvg_adam_step_segments_clip      (coef 0.37 and 1)     1.03 .. 1.887  12  0.79 .. 1.958   8   0.77 .. 1.468   8   1.1e-07 .. 3.2e-03
  mvg_adam_step_segments_dev_clip  (coef 0.37 and 1)     1.03 .. 1.887  12  0.79 .. 1.958   8   0.77 .. 1.468   8   1.1e-07 .. 3.2e-03
  mvg_adam_step, 20 teacher-forced steps                 1.59 .. 1.897  12  1.17 .. 1.937   8   0.96 .. 1.179   8   6.4e-05 .. 5.9e-04
  mvg_adam_step_segments_dev, 20 teacher-forced steps    1.50 .. 1.865  12  1.06 .. 1.952   8   0.89 .. 1.150   8   1.7e-04 .. 9.8e-03
  adam_tick_kernel / adam_tick_segments_kernel without a record / with one: 37 / 201 / 282 rows, every bc1 and sqrt(bc2) the
  float32 nearest to the float64 value (0 ulp; the bar is 1), every count exact
The kernel sits at the float32 restatement's own level (2.9 / 2.0 / 1.8 units on the CPU) and below it on m, where the compiler
contracts b1 * m + (1 - b1) * g_r into a fused multiply-add.  The segmented forms print the same figures as each other - they run
the same adam_elem on the same bits - and the unclipped ones the same as the clipped ones at coef = 1.  The step max-rel column is what
the parameter-relative anchor never saw; it is large (1e-3) only where the largest step of a segment is itself small against |p|,
i.e. where it measures the rounding of p' - the units account for that, the column does not.
The sub-normal case: (1 - b2) g^2 = 1e-42 is kept, not flushed, on all 1020 elements; |p'| reaches 0.99999998 of its bound."""
import numpy as np
import pytest
import torch

import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd import ops

import adam_forms_ref as R
from adam_forms_ref import HYPER, K_M, K_P, K_V
from grad_clip_ref import within_one_ulp

pytestmark = pytest.mark.gpu

JUNK = (7.5, -3.25)                                  # what a state row holds behind its count before the tick


def dev():
    return torch.device("cuda:0")


def up(a):
    """A float32 array on the device with every bit as it is (NaN payloads included)."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(dev()).view(torch.float32)


def down(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().view(np.float32)


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def flat():
    """[(arena, references)] of the 36 one-segment problems, computed once for both plain entry points."""
    return cached("flat", lambda: [(a, a.references()) for a in R.flat_arenas()])


def segmented():
    """[(arena, references)] of the segmented problems without clipping (coef = 1 gives the same bits), computed once."""
    return cached("segmented", lambda: [(a, a.references()) for a in R.segment_arenas()])


class Failures(list):
    def check(self, ok, what):
        if not ok:
            self.append(what)

    def done(self):
        assert not self, "\n".join(self)


def hold(fails, entry, case, arena, refs, got, p_before=None):
    """Print the line of one comparison and note what is outside the bars; got = (p, m, v) as float32 arrays."""
    (wm, wv, wp), rel = arena.compare(refs, got[0], got[1], got[2], p_before=p_before)
    print(f"ADAM-FORMS {entry} {case}: m {wm:.3f} v {wv:.3f} p {wp:.3f}   step max-rel {rel:.3e}")
    fails.check(all(np.isfinite(x) for x in (wm, wv, wp)), f"{entry} {case}: an output inside a segment is not finite")
    fails.check(wm <= K_M and wv <= K_V and wp <= K_P, f"{entry} {case}: m {wm:.3f} (K {K_M}) v {wv:.3f} (K {K_V}) p {wp:.3f} (K {K_P})")


def hold_outside(fails, entry, case, arena, p, g, m, v):
    mask = arena.outside()
    if mask.any():
        for got, old, what in zip((p, g, m, v), (arena.p, arena.g, arena.m, arena.v), ("param", "grad", "exp_avg", "exp_avg_sq")):
            fails.check(same_bits(down(got)[mask], old[mask]), f"{entry} {case}: {what} outside the segments changed")


def ulps(got, want64):
    """Distance in float32 steps between got and the float64 want rounded to float32 (both positive and finite here)."""
    return abs(int(np.float32(got).view(np.int32)) - int(np.float32(want64).view(np.int32)))


def hold_rows(fails, tick, case, rows, wants):
    """rows: the device table after the call; wants: [(step, b1, b2)] per row."""
    rows = down(rows).reshape(-1, 3)
    worst = [0, 0]
    for k, (row, (step, b1, b2)) in enumerate(zip(rows, wants)):
        want = R.state_row(step, b1, b2)
        fails.check(float(row[0]) == float(step), f"{tick} {case}: row {k} counts {row[0]} after the tick, not {step}")
        for i in (1, 2):
            fails.check(within_one_ulp(row[i], np.float32(want[i])), f"{tick} {case}: row {k}[{i}] = {row[i]!r}, wanted {want[i]!r}")
            worst[i - 1] = max(worst[i - 1], ulps(row[i], want[i]))
    print(f"ADAM-FORMS {tick} {case}: {len(wants)} row(s), step exact, bc1 {worst[0]} ulp, sqrt(bc2) {worst[1]} ulp")


def rows_before(steps):
    return torch.tensor([[float(s - 1), JUNK[0], JUNK[1]] for s in steps], dtype=torch.float32).reshape(-1, 3).to(dev())


def host_records(arena, lrs=None):
    """(begin, end, lr, b1, b2, eps, wd, step) of ops.adam_step_segments."""
    out = []
    for k, (b, e, h) in enumerate(arena.segs):
        lr, b1, b2, eps, wd, step = HYPER[h]
        if lrs is not None:
            lr, step = lrs[k]
        out.append((b, e, lr, b1, b2, eps, wd, step))
    return out


def dev_records(arena):
    """(begin, end, lr_index, b1, b2, eps, wd) of ops.adam_step_segments_dev, reading R.lr_table()."""
    return [(b, e, R.lr_index(h)) + HYPER[h][1:5] for b, e, h in arena.segs]


def tensors(arena):
    return up(arena.p), up(arena.g), up(arena.m), up(arena.v)


# ---------------------------------------------------------------- the two plain entry points
def run_plain(entry, arena):
    """One call of ops.adam_step / ops.adam_step_dev on a one-segment arena: (p, g, m, v, state row or None)."""
    (b, e, h), = arena.segs
    lr, b1, b2, eps, wd, step = HYPER[h]
    p, g, m, v = tensors(arena)
    if entry == "adam_step":
        ops.adam_step(p, g, m, v, lr, b1, b2, eps, wd, step)
        return p, g, m, v, None
    state = rows_before([step]).reshape(3)
    ops.adam_step_dev(p, g, m, v, up(np.array([lr], dtype=np.float32)), state, b1, b2, eps, wd)
    return p, g, m, v, state


@pytest.mark.parametrize("entry", ["adam_step", "adam_step_dev"])
def test_plain_entry_points_at_every_hyper_set_scale_and_size(entry):
    fails = Failures()
    for arena, refs in flat():
        p, g, m, v, state = run_plain(entry, arena)
        hold(fails, entry, arena.name, arena, refs, (down(p), down(m), down(v)))
        fails.check(same_bits(down(g), arena.g), f"{entry} {arena.name}: the gradient changed")
        if state is not None:
            h = arena.segs[0][2]
            hold_rows(fails, "adam_tick", arena.name, state, [(HYPER[h][5], HYPER[h][1], HYPER[h][2])])
    fails.done()


@pytest.mark.parametrize("entry", ["adam_step", "adam_step_dev"])
def test_plain_entry_points_past_the_grid_cap(entry):
    """n / 4 = 8192 * 256 + 128 slots: every lane of the capped grid takes one slot, the first 128 a second one."""
    arena = R.big_arena(entry)
    assert arena.n // 4 == 8192 * 256 + 128
    fails = Failures()
    p, g, m, v, state = run_plain(entry, arena)
    hold(fails, entry, arena.name, arena, arena.references(), (down(p), down(m), down(v)))
    if state is not None:
        h = arena.segs[0][2]
        hold_rows(fails, "adam_tick", arena.name, state, [(HYPER[h][5], HYPER[h][1], HYPER[h][2])])
    fails.done()


# ---------------------------------------------------------------- the four segmented entry points
def record_for(arena, g, mode):
    """The clip4 record of one clipped call and the coefficient the reference takes: written by ops.grad_norm_segments for a
    max_norm of 0.37 of the norm ("norm"), by hand with coef = 1 ("one"), or by hand with the skipped flag set ("skipped")."""
    if mode == "norm":
        max_norm, want = arena.clip()
        clip4 = torch.zeros(4, device=dev())
        ops.grad_norm_segments(g, [(b, e) for b, e, _ in arena.segs], max_norm, True, clip4)
        rec = down(clip4)
        assert rec[2] == 0.0 and rec[1] < 1.0 and within_one_ulp(rec[1], np.float32(want)), (rec, want)
        return clip4, float(rec[1])
    if mode == "one":
        return up(np.array([3.0, 1.0, 0.0, 0.0], dtype=np.float32)), 1.0
    return up(np.array([np.nan, 0.0, 1.0, 5.0], dtype=np.float32)), None


def run_segmented(entry, arena, clip4):
    """One call of the segmented entry point `entry`: (p, g, m, v, state rows or None)."""
    p, g, m, v = tensors(arena)
    state = None
    if entry == "adam_step_segments":
        ops.adam_step_segments(p, g, m, v, host_records(arena))
    elif entry == "adam_step_segments_clip":
        ops.adam_step_segments_clip(p, g, m, v, host_records(arena), clip4)
    else:
        state = rows_before([HYPER[h][5] for _, _, h in arena.segs])
        lr_dev = up(np.array(R.lr_table(), dtype=np.float32))
        if entry == "adam_step_segments_dev":
            ops.adam_step_segments_dev(p, g, m, v, dev_records(arena), lr_dev, state)
        else:
            ops.adam_step_segments_dev_clip(p, g, m, v, dev_records(arena), lr_dev, state, clip4)
    return p, g, m, v, state


TICK = {"adam_step_segments_dev": "adam_tick_segments", "adam_step_segments_dev_clip": "adam_tick_segments_clip"}


@pytest.mark.parametrize("entry,mode", [("adam_step_segments", None), ("adam_step_segments_dev", None),
                                        ("adam_step_segments_clip", "norm"), ("adam_step_segments_clip", "one"),
                                        ("adam_step_segments_dev_clip", "norm"), ("adam_step_segments_dev_clip", "one")])
def test_segmented_entry_points_on_both_layouts(entry, mode):
    fails = Failures()
    for arena, refs in segmented():
        case = arena.name + ("" if mode is None else "_coef1" if mode == "one" else "_clipped")
        clip4 = None
        if mode is not None:
            clip4, coef = record_for(arena, up(arena.g), mode)
            if mode == "norm":
                refs = arena.references(coef=coef)
        p, g, m, v, state = run_segmented(entry, arena, clip4)
        hold(fails, entry, case, arena, refs, (down(p), down(m), down(v)))
        hold_outside(fails, entry, case, arena, p, g, m, v)
        fails.check(same_bits(down(g), arena.g), f"{entry} {case}: the gradient changed")
        if state is not None:
            hold_rows(fails, TICK[entry], case, state, [(HYPER[h][5], HYPER[h][1], HYPER[h][2]) for _, _, h in arena.segs])
    fails.done()


@pytest.mark.parametrize("entry", ["adam_step_segments_clip", "adam_step_segments_dev_clip"])
def test_a_skipped_step_leaves_every_bit(entry):
    for arena, _ in segmented()[::4]:
        clip4, _ = record_for(arena, None, "skipped")
        before_rows = down(rows_before([HYPER[h][5] for _, _, h in arena.segs])).copy()
        p, g, m, v, state = run_segmented(entry, arena, clip4)
        for got, old, what in zip((p, g, m, v), (arena.p, arena.g, arena.m, arena.v), ("param", "grad", "exp_avg", "exp_avg_sq")):
            assert same_bits(down(got), old), f"{entry} {arena.name}: {what} changed in a skipped step"
        if state is not None:
            assert same_bits(down(state), before_rows), f"{entry} {arena.name}: a state row advanced in a skipped step"
        assert same_bits(down(clip4), np.array([np.nan, 0.0, 1.0, 5.0], dtype=np.float32))
        print(f"ADAM-FORMS {entry} {arena.name}_skipped: p, g, m, v and the rows bit for bit")


# ---------------------------------------------------------------- twenty teacher-forced steps
def test_twenty_teacher_forced_steps_of_adam_step():
    lr0, b1, b2, eps, wd, _ = HYPER[1]
    arena = R.Arena("sequence_n4100", 4100, [(0, 4100, 1)], 1.0, seed=801)
    arena.m[:] = 0
    arena.v[:] = 0
    p, _, m, v = tensors(arena)
    fails = Failures()
    for step in range(1, 21):
        arena.g[:] = R.sequence_gradient(4100, step)
        lr = R.sequence_lr(lr0, step)
        before = (down(p).copy(), down(m).copy(), down(v).copy())
        ops.adam_step(p, up(arena.g), m, v, lr, b1, b2, eps, wd, step)
        refs = arena.references(state=before, lrs=[(lr, step)])
        hold(fails, "adam_step", f"sequence_n4100_step{step:02d}", arena, refs, (down(p), down(m), down(v)), p_before=before[0])
    fails.done()


def test_twenty_teacher_forced_steps_of_adam_step_segments_dev():
    arena = R.sequence_arena()
    p, _, m, v = tensors(arena)
    state = rows_before([1] * len(arena.segs))
    table = np.array(R.lr_table(), dtype=np.float32)
    fails = Failures()
    for step in range(1, 21):
        lrs = []
        for b, e, h in arena.segs:
            arena.g[b:e] = R.sequence_gradient(e - b, step, seed=820 + h)
            table[R.lr_index(h)] = R.sequence_lr(HYPER[h][0], step + h)            # the host rewrites the table between steps
            lrs.append((float(table[R.lr_index(h)]), step))
        before = (down(p).copy(), down(m).copy(), down(v).copy())
        g = up(arena.g)
        ops.adam_step_segments_dev(p, g, m, v, dev_records(arena), up(table), state)
        case = f"sequence_n4100_step{step:02d}"
        hold(fails, "adam_step_segments_dev", case, arena, arena.references(state=before, lrs=lrs), (down(p), down(m), down(v)),
             p_before=before[0])
        hold_rows(fails, "adam_tick_segments", case, state, [(step, HYPER[h][1], HYPER[h][2]) for _, _, h in arena.segs])
        mask = arena.outside()
        for got, old in zip((p, m, v), (arena.p, arena.m, arena.v)):
            fails.check(same_bits(down(got)[mask], old[mask]), f"{case}: something outside the segments changed")
    fails.done()


# ---------------------------------------------------------------- exact cases
@pytest.mark.parametrize("entry", ["adam_step", "adam_step_dev", "adam_step_segments", "adam_step_segments_dev"])
def test_zero_gradient_and_moments_without_weight_decay_change_nothing(entry):
    h = 3
    assert HYPER[h][4] == 0.0
    arena = R.Arena("zeros_n1020", 1020, [(0, 1020, h)], 1.0, seed=830)
    arena.g[:] = 0
    arena.m[:] = 0
    arena.v[:] = 0
    p, g, m, v, _ = run_plain(entry, arena) if entry in ("adam_step", "adam_step_dev") else run_segmented(entry, arena, None)
    assert same_bits(down(p), arena.p) and same_bits(down(m), arena.m) and same_bits(down(v), arena.v)
    print(f"ADAM-FORMS {entry} zeros_n1020: p, m, v bit for bit")


@pytest.mark.parametrize("entry", ["adam_step", "adam_step_segments"])
def test_a_nan_gradient_stays_in_its_own_lane(entry):
    h = 1
    arena = R.Arena("nan_lanes_n1020", 1020, [(0, 1020, h)], 1.0, seed=831)
    clean = arena.g.copy()
    lanes = [4 * 3 + 0, 4 * 100 + 1, 4 * 101 + 2, 4 * 254 + 3]                         # x, y, z, w of different slots (the last slot's w)
    arena.g[lanes] = np.nan
    p, g, m, v, _ = run_plain(entry, arena) if entry == "adam_step" else run_segmented(entry, arena, None)
    got = [down(t).copy() for t in (p, m, v)]
    want_nan = np.zeros(1020, dtype=bool)
    want_nan[lanes] = True
    for arr, what in zip(got, ("param", "exp_avg", "exp_avg_sq")):
        assert np.array_equal(np.isnan(arr), want_nan), f"{entry}: NaN elements of {what}: {np.flatnonzero(np.isnan(arr)).tolist()}"
    # everything else, the three slot neighbours of each NaN included, against the reference of the clean gradient
    arena.g[:] = clean
    refs = arena.references()
    for arr, key in zip(got, ("p", "m", "v")):
        arr[lanes] = refs[0][key][lanes].astype(np.float32)
    fails = Failures()
    hold(fails, entry, arena.name, arena, refs, got)
    fails.done()


@pytest.mark.parametrize("entry", ["adam_step", "adam_step_dev"])
def test_subnormal_second_moment(entry):
    """|g| = 1e-20 from zero state: (1 - b2) g^2 = 1e-42 is sub-normal.  Whether the hardware keeps or flushes it, sqrt(v) / sqrt(bc2) is
    far below eps, so the outputs are finite and |p'| <= (lr / bc1) |m'| / eps - up to the three float32 roundings of lr / bc1, m / denom
    and their product, with m' the kernel's own."""
    h = 3
    lr, b1, b2, eps, wd, _ = R.hyper32(h)
    arena = R.Arena("subnormal_n1020", 1020, [(0, 1020, h)], 0.0, seed=832)
    arena.g[:] = np.where(arena.g > 0, np.float32(1e-20), np.float32(-1e-20))
    arena.m[:] = 0
    arena.v[:] = 0
    HY = list(HYPER[h])
    p, g, m, v = tensors(arena)
    if entry == "adam_step":
        ops.adam_step(p, g, m, v, HY[0], HY[1], HY[2], HY[3], HY[4], 1)
    else:
        state = rows_before([1]).reshape(3)
        ops.adam_step_dev(p, g, m, v, up(np.array([HY[0]], dtype=np.float32)), state, HY[1], HY[2], HY[3], HY[4])
    p, m, v = (down(t).astype(np.float64) for t in (p, m, v))
    assert np.isfinite(p).all() and np.isfinite(m).all() and np.isfinite(v).all()
    assert (m != 0).all() and (p != 0).all() and (v >= 0).all() and (np.sign(p) == -np.sign(arena.g)).all()
    bound = (lr / (1.0 - b1)) * np.abs(m) / eps
    worst = float((np.abs(p) / bound).max())
    print(f"ADAM-FORMS {entry} subnormal_n1020: finite, largest |p'| / ((lr / bc1) |m'| / eps) {worst:.9f}, v' kept on "
          f"{int((v != 0).sum())} of 1020 elements")
    assert worst <= 1.0 + 3 * 2.0 ** -24
