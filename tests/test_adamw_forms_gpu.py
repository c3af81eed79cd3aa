"""Every entry point of decoupled weight decay in csrc/adam.hip called directly (ops.*) and held, element by element, to the
float64 statement of one torch.optim.AdamW step in tests/adamw_forms_ref.py - the parameter, both moments and, for the device
forms, the state rows their tick kernels advance.  Runs on an MI355X only; the reference, its units, the bars and the table's
sensitivity are checked without a GPU in tests/test_adamw_forms_cpu.py.

An element passes when |got - want| <= K * 2^-24 * U with the propagated units U_m, U_v, U_p of the reference and K_M = 8,
K_V = 8, K_P = 7: four times what the same operation order costs in NumPy float32, measured on the CPU over this very table and
never re-fitted to the kernel.  Every comparison prints
    ADAMW-FORMS <entry> <case>: m <units> v <units> p <units>   step max-rel <max |d_got - d_ref| / max |d_ref|>
before it asserts the outputs finite and inside the bars (every line of an MI355X run: profiles/adamw_forms_errors.txt); the
device forms add a line for their tick kernel.  Holes of the segmented arenas hold distinct NaN patterns in p, g, m and v and must
come back bit for bit; a skipped step must leave everything bit for bit, the rows included.

Cases (adam_forms_ref's table): mvg_adamw_step and mvg_adamw_step_dev on the 36 flat problems and once each on
n = 8192 * 256 * 4 + 512; mvg_adam_step_segments_ex and mvg_adam_step_segments_dev_ex on both three-segment layouts at six rotations
and on 35 segments in three launches, every segment decoupled, with a NULL record, a record mvg_grad_norm_segments wrote (coef
0.37) and a hand-written coef = 1; the 35 segments with the modes alternating, where the coupled segments must equal the four
existing segmented entry points bit for bit and the decoupled ones meet the bars.  Bit relations: a decoupled segment of _ex is
mvg_adamw_step over that slice, one of _dev_ex is mvg_adamw_step_dev with a one-element lr_dev and the same row, a NULL record is
coef = 1, and on the hyper set without weight decay decoupled is coupled.  Twenty teacher-forced steps of mvg_adamw_step and
mvg_adam_step_segments_dev_ex with a learning rate that changes every step, each held to the reference evaluated from the kernel's
own previous state.

Measured on an MI355X (every line: profiles/adamw_forms_errors.txt), smallest .. largest units over the cases, next to K:
  entry point                                            m             K_M   v              K_V   p              K_P   step max-rel
  mvg_adamw_step               (36 cases)                0 .. 1.92     8     0.29 .. 1.91   8     0.18 .. 1.28   7     1.6e-08 .. 4.8e-04
  mvg_adamw_step               n = 8192 * 256 * 4 + 512  1.95          8     1.98           8     1.11           7     5.2e-06
  mvg_adamw_step_dev           (36 cases)                0 .. 1.92     8     0.29 .. 1.91   8     0.18 .. 1.28   7     1.6e-08 .. 4.8e-04
  mvg_adamw_step_dev           n = 8192 * 256 * 4 + 512  1.99          8     1.99           8     1.62           7     9.6e-08
  mvg_adam_step_segments_ex      NULL record (15)        0.97 .. 1.79  8     0.79 .. 1.89   8     0.49 .. 1.18   7     1.1e-07 .. 1.4e-03
  mvg_adam_step_segments_ex      coef 0.37 and 1 (30)    0.97 .. 1.87  8     0.79 .. 1.96   8     0.49 .. 1.18   7     1.1e-07 .. 3.2e-03
  mvg_adam_step_segments_ex      mixed modes (6)         0.89 .. 1.67  8     1.36 .. 1.83   8     0.75 .. 0.99   7     1.4e-07 .. 1.0e-04
  mvg_adam_step_segments_dev_ex  the same 51 cases: the same figures in every digit (the same adam_elem<true> on the same bits)
  mvg_adamw_step, 20 teacher-forced steps                0.95 .. 1.90  8     0.60 .. 1.94   8     0.90 .. 1.13   7     2.7e-04 .. 1.9e-03
  mvg_adam_step_segments_dev_ex, 20 teacher-forced steps 0.94 .. 1.84  8     0.58 .. 1.93   8     0.91 .. 1.13   7     4.1e-04 .. 9.8e-03
  the ticks: 108 lines of rows, every bc1 and sqrt(bc2) the float32 nearest to the float64 value (0 ulp; the bar is 1), every count exact
The kernels sit at the float32 restatement's own level (1.99 / 1.99 / 1.71 units on the CPU, on the same n = 8.4 M problem).  The step
max-rel column counts the decay's share of the move (adamw_forms_ref.step_max_rel)."""
import numpy as np
import pytest
import torch

import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd import ops

import adam_forms_ref as R
import adamw_forms_ref as W
from adam_forms_ref import HYPER
from adamw_forms_ref import K_M, K_P, K_V
from grad_clip_ref import within_one_ulp

pytestmark = pytest.mark.gpu

JUNK = (7.5, -3.25)                                  # what a state row holds behind its count before the tick
HOST_EX, DEV_EX = "adam_step_segments_ex", "adam_step_segments_dev_ex"


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
    """[(arena, decoupled references)] of the 36 one-segment problems, computed once for both plain entry points."""
    return cached("flat", lambda: [(a, W.references(a)) for a in R.flat_arenas()])


def segmented():
    """[(arena, decoupled references)] of the segmented problems without clipping (coef = 1 gives the same bits), computed once."""
    return cached("segmented", lambda: [(a, W.references(a)) for a in R.segment_arenas()])


def thirty_five():
    return [a for a, _ in segmented() if a.name.startswith("thirty_five")]


class Failures(list):
    def check(self, ok, what):
        if not ok:
            self.append(what)

    def done(self):
        assert not self, "\n".join(self)


def hold(fails, entry, case, arena, refs, got, p_before=None, modes=None):
    """Print the line of one comparison over the decoupled segments and note what is outside the bars; got = (p, m, v)."""
    p_before = arena.p if p_before is None else p_before
    worst, rel = [0.0, 0.0, 0.0], 0.0
    for k, ((b, e, _), r) in enumerate(zip(arena.segs, refs)):
        if modes is not None and not modes[k]:
            continue
        w = R.worst_units(r, got[0][b:e], got[1][b:e], got[2][b:e])
        worst = [x if (x != x or x >= y) else y for x, y in zip(w, worst)]
        rel = max(rel, W.step_max_rel(r, p_before[b:e], got[0][b:e]))
    wm, wv, wp = worst
    print(f"ADAMW-FORMS {entry} {case}: m {wm:.3f} v {wv:.3f} p {wp:.3f}   step max-rel {rel:.3e}")
    fails.check(all(np.isfinite(x) for x in (wm, wv, wp)), f"{entry} {case}: an output inside a segment is not finite")
    fails.check(wm <= K_M and wv <= K_V and wp <= K_P, f"{entry} {case}: m {wm:.3f} (K {K_M}) v {wv:.3f} (K {K_V}) p {wp:.3f} (K {K_P})")


def hold_outside(fails, entry, case, arena, p, g, m, v):
    mask = arena.outside()
    if mask.any():
        for got, old, what in zip((p, g, m, v), (arena.p, arena.g, arena.m, arena.v), ("param", "grad", "exp_avg", "exp_avg_sq")):
            fails.check(same_bits(down(got)[mask], old[mask]), f"{entry} {case}: {what} outside the segments changed")


def ulps(got, want64):
    return abs(int(np.float32(got).view(np.int32)) - int(np.float32(want64).view(np.int32)))


def hold_rows(fails, tick, case, rows, wants):
    """rows: the device table after the call; wants: [(step, b1, b2)] per row (the Adam test's rule: step exact, one ulp)."""
    rows = down(rows).reshape(-1, 3)
    worst = [0, 0]
    for k, (row, (step, b1, b2)) in enumerate(zip(rows, wants)):
        want = R.state_row(step, b1, b2)
        fails.check(float(row[0]) == float(step), f"{tick} {case}: row {k} counts {row[0]} after the tick, not {step}")
        for i in (1, 2):
            fails.check(within_one_ulp(row[i], np.float32(want[i])), f"{tick} {case}: row {k}[{i}] = {row[i]!r}, wanted {want[i]!r}")
            worst[i - 1] = max(worst[i - 1], ulps(row[i], want[i]))
    print(f"ADAMW-FORMS {tick} {case}: {len(wants)} row(s), step exact, bc1 {worst[0]} ulp, sqrt(bc2) {worst[1]} ulp")


def rows_before(steps):
    return torch.tensor([[float(s - 1), JUNK[0], JUNK[1]] for s in steps], dtype=torch.float32).reshape(-1, 3).to(dev())


def row_wants(arena):
    return [(HYPER[h][5], HYPER[h][1], HYPER[h][2]) for _, _, h in arena.segs]


def host_records(arena, modes=None, lrs=None):
    """(begin, end, lr, b1, b2, eps, wd, step[, mode]) of ops.adam_step_segments[_clip] (modes None) / ops.adam_step_segments_ex."""
    out = []
    for k, (b, e, h) in enumerate(arena.segs):
        lr, b1, b2, eps, wd, step = HYPER[h]
        if lrs is not None:
            lr, step = lrs[k]
        out.append((b, e, lr, b1, b2, eps, wd, step) + (() if modes is None else (modes[k],)))
    return out


def dev_records(arena, modes=None):
    """(begin, end, lr_index, b1, b2, eps, wd[, mode]) of ops.adam_step_segments_dev[_clip] / _dev_ex, reading R.lr_table()."""
    return [(b, e, R.lr_index(h)) + HYPER[h][1:5] + (() if modes is None else (modes[k],)) for k, (b, e, h) in enumerate(arena.segs)]


def tensors(arena):
    return up(arena.p), up(arena.g), up(arena.m), up(arena.v)


def lr_table():
    return up(np.array(R.lr_table(), dtype=np.float32))


# ---------------------------------------------------------------- the two plain entry points
def run_plain(entry, arena):
    """One call of ops.adamw_step / adamw_step_dev (or their coupled twins) on a one-segment arena: (p, g, m, v, row or None)."""
    (b, e, h), = arena.segs
    lr, b1, b2, eps, wd, step = HYPER[h]
    p, g, m, v = tensors(arena)
    if entry in ("adamw_step", "adam_step"):
        getattr(ops, entry)(p, g, m, v, lr, b1, b2, eps, wd, step)
        return p, g, m, v, None
    state = rows_before([step]).reshape(3)
    getattr(ops, entry)(p, g, m, v, up(np.array([lr], dtype=np.float32)), state, b1, b2, eps, wd)
    return p, g, m, v, state


@pytest.mark.parametrize("entry", ["adamw_step", "adamw_step_dev"])
def test_plain_entry_points_at_every_hyper_set_scale_and_size(entry):
    fails = Failures()
    for arena, refs in flat():
        p, g, m, v, state = run_plain(entry, arena)
        hold(fails, entry, arena.name, arena, refs, (down(p), down(m), down(v)))
        fails.check(same_bits(down(g), arena.g), f"{entry} {arena.name}: the gradient changed")
        if state is not None:
            hold_rows(fails, "adam_tick", arena.name, state, row_wants(arena))
    fails.done()


@pytest.mark.parametrize("entry", ["adamw_step", "adamw_step_dev"])
def test_plain_entry_points_past_the_grid_cap(entry):
    """n / 4 = 8192 * 256 + 128 slots: every lane of the capped grid takes one slot, the first 128 a second one."""
    arena = R.big_arena(entry.replace("adamw", "adam"))
    assert arena.n // 4 == 8192 * 256 + 128
    fails = Failures()
    p, g, m, v, state = run_plain(entry, arena)
    hold(fails, entry, arena.name, arena, W.references(arena), (down(p), down(m), down(v)))
    if state is not None:
        hold_rows(fails, "adam_tick", arena.name, state, row_wants(arena))
    fails.done()


# ---------------------------------------------------------------- the two segmented entry points, every segment decoupled
def record_for(arena, mode):
    """The clip4 record of one call and the coefficient the reference takes: None (a NULL record), written by
    ops.grad_norm_segments for a max_norm of 0.37 of the norm ("norm"), by hand with coef = 1 ("one") or with the skipped flag set
    ("skipped")."""
    if mode is None:
        return None, None
    if mode == "norm":
        max_norm, want = arena.clip()
        clip4 = torch.zeros(4, device=dev())
        ops.grad_norm_segments(up(arena.g), [(b, e) for b, e, _ in arena.segs], max_norm, True, clip4)
        rec = down(clip4)
        assert rec[2] == 0.0 and rec[1] < 1.0 and within_one_ulp(rec[1], np.float32(want)), (rec, want)
        return clip4, float(rec[1])
    if mode == "one":
        return up(np.array([3.0, 1.0, 0.0, 0.0], dtype=np.float32)), None
    return up(np.array([np.nan, 0.0, 1.0, 5.0], dtype=np.float32)), None


def run_ex(entry, arena, modes, clip4):
    """One call of ops.adam_step_segments_ex / _dev_ex: (p, g, m, v, state rows or None)."""
    p, g, m, v = tensors(arena)
    if entry == HOST_EX:
        ops.adam_step_segments_ex(p, g, m, v, host_records(arena, modes), clip4)
        return p, g, m, v, None
    state = rows_before([HYPER[h][5] for _, _, h in arena.segs])
    ops.adam_step_segments_dev_ex(p, g, m, v, dev_records(arena, modes), lr_table(), state, clip4)
    return p, g, m, v, state


def run_coupled(entry, arena, clip4):
    """The existing entry point that `entry` with this record must equal on coupled segments."""
    p, g, m, v = tensors(arena)
    if entry == HOST_EX:
        if clip4 is None:
            ops.adam_step_segments(p, g, m, v, host_records(arena))
        else:
            ops.adam_step_segments_clip(p, g, m, v, host_records(arena), clip4)
        return p, g, m, v, None
    state = rows_before([HYPER[h][5] for _, _, h in arena.segs])
    if clip4 is None:
        ops.adam_step_segments_dev(p, g, m, v, dev_records(arena), lr_table(), state)
    else:
        ops.adam_step_segments_dev_clip(p, g, m, v, dev_records(arena), lr_table(), state, clip4)
    return p, g, m, v, state


def case_of(arena, mode):
    return arena.name + {None: "", "one": "_coef1", "norm": "_clipped", "skipped": "_skipped"}[mode]


@pytest.mark.parametrize("mode", [None, "norm", "one"])
@pytest.mark.parametrize("entry", [HOST_EX, DEV_EX])
def test_segmented_entry_points_with_every_segment_decoupled(entry, mode):
    fails = Failures()
    for arena, refs in segmented():
        case = case_of(arena, mode)
        clip4, coef = record_for(arena, mode)
        if coef is not None:
            refs = W.references(arena, coef=coef)
        p, g, m, v, state = run_ex(entry, arena, [1] * len(arena.segs), clip4)
        hold(fails, entry, case, arena, refs, (down(p), down(m), down(v)))
        hold_outside(fails, entry, case, arena, p, g, m, v)
        fails.check(same_bits(down(g), arena.g), f"{entry} {case}: the gradient changed")
        if state is not None:
            hold_rows(fails, "adam_tick_segments" + ("" if clip4 is None else "_clip"), case, state, row_wants(arena))
    fails.done()


@pytest.mark.parametrize("entry", [HOST_EX, DEV_EX])
def test_a_skipped_step_leaves_every_bit(entry):
    for arena, _ in segmented()[::4]:
        clip4, _ = record_for(arena, "skipped")
        before_rows = down(rows_before([HYPER[h][5] for _, _, h in arena.segs])).copy()
        p, g, m, v, state = run_ex(entry, arena, [(k + 1) % 2 for k in range(len(arena.segs))], clip4)
        for got, old, what in zip((p, g, m, v), (arena.p, arena.g, arena.m, arena.v), ("param", "grad", "exp_avg", "exp_avg_sq")):
            assert same_bits(down(got), old), f"{entry} {arena.name}: {what} changed in a skipped step"
        if state is not None:
            assert same_bits(down(state), before_rows), f"{entry} {arena.name}: a state row advanced in a skipped step"
        assert same_bits(down(clip4), np.array([np.nan, 0.0, 1.0, 5.0], dtype=np.float32))
        print(f"ADAMW-FORMS {entry} {arena.name}_skipped: p, g, m, v and the rows bit for bit")


# ---------------------------------------------------------------- coupled and decoupled segments in one launch
@pytest.mark.parametrize("mode", [None, "norm"])
@pytest.mark.parametrize("entry", [HOST_EX, DEV_EX])
def test_mixed_launch_of_35_segments_with_alternating_modes(entry, mode):
    """Three launches of 16 + 16 + 3 segments, each holding both modes: segment i is decoupled when i is even.  mode None pairs
    with mvg_adam_step_segments (_dev), "norm" with mvg_adam_step_segments_clip (_dev_clip)."""
    fails = Failures()
    for arena in thirty_five():
        modes = [(i + 1) % 2 for i in range(len(arena.segs))]
        case = case_of(arena, mode) + "_mixed"
        clip4, coef = record_for(arena, mode)
        refs = W.references(arena, coef=coef, modes=modes)
        p, g, m, v, state = run_ex(entry, arena, modes, clip4)
        got = (down(p), down(m), down(v))
        hold(fails, entry, case, arena, refs, got, modes=modes)
        hold_outside(fails, entry, case, arena, p, g, m, v)
        cp, _, cm, cv, cstate = run_coupled(entry, arena, clip4)
        twin = (down(cp), down(cm), down(cv))
        differs = 0
        for k, (b, e, h) in enumerate(arena.segs):
            if modes[k]:
                differs += HYPER[h][4] != 0.0 and arena.scale != 0.0 and not same_bits(got[0][b:e], twin[0][b:e])
                continue
            for x, y, what in zip(got, twin, ("param", "exp_avg", "exp_avg_sq")):
                fails.check(same_bits(x[b:e], y[b:e]), f"{entry} {case}: {what} of coupled segment {k} is not the coupled entry point's")
        if arena.scale != 0.0:
            fails.check(differs > 0, f"{entry} {case}: no decoupled segment differs from the coupled entry point")
        if state is not None:
            hold_rows(fails, "adam_tick_segments" + ("" if clip4 is None else "_clip"), case, state, row_wants(arena))
            fails.check(same_bits(down(state), down(cstate)), f"{entry} {case}: the rows are not the coupled entry point's")
        print(f"ADAMW-FORMS {entry} {case}: {modes.count(0)} coupled segments bit for bit the coupled entry point's")
    fails.done()


# ---------------------------------------------------------------- bit relations
@pytest.mark.parametrize("entry", [HOST_EX, DEV_EX])
def test_a_decoupled_segment_is_the_plain_entry_point_over_its_slice(entry):
    plain = "adamw_step" if entry == HOST_EX else "adamw_step_dev"
    picked = [a for a, _ in segmented() if a.name.startswith("three")][::3] + thirty_five()[:1]
    count = 0
    for arena in picked:
        p, g, m, v, state = run_ex(entry, arena, [1] * len(arena.segs), None)
        got = (down(p), down(m), down(v))
        rows = None if state is None else down(state).reshape(-1, 3)
        for k, (b, e, _) in enumerate(arena.segs[:8]):
            sp, _, sm, sv, srow = run_plain(plain, W.slice_arena(arena, k))
            for x, y, what in zip(got, (down(sp), down(sm), down(sv)), ("param", "exp_avg", "exp_avg_sq")):
                assert same_bits(x[b:e], y), f"{entry} {arena.name}: {what} of segment {k} is not {plain}'s over the slice"
            if rows is not None:
                assert same_bits(rows[k], down(srow)), f"{entry} {arena.name}: row {k} is not {plain}'s"
            count += 1
    print(f"ADAMW-FORMS {entry}: {count} decoupled segments of {len(picked)} arenas bit for bit {plain} over their slices")


@pytest.mark.parametrize("entry", [HOST_EX, DEV_EX])
def test_a_null_record_is_coef_1(entry):
    for arena, _ in segmented()[::4] + [(a, None) for a in thirty_five()[1:2]]:
        modes = [(k + 1) % 2 for k in range(len(arena.segs))]
        a = run_ex(entry, arena, modes, None)
        b = run_ex(entry, arena, modes, record_for(arena, "one")[0])
        for x, y in zip(a, b):
            assert (x is None and y is None) or same_bits(down(x), down(y)), f"{entry} {arena.name}: NULL clip4 and coef = 1 differ"
        print(f"ADAMW-FORMS {entry} {arena.name}: a NULL record and coef = 1 agree in every bit")


def test_without_weight_decay_decoupled_is_coupled():
    h = 3
    assert HYPER[h][4] == 0.0
    count = 0
    for arena, _ in flat():
        if arena.segs[0][2] != h:
            continue
        for entry in ("adamw_step", "adamw_step_dev"):
            a, b = run_plain(entry, arena), run_plain(entry.replace("adamw", "adam"), arena)
            for x, y in zip(a, b):
                assert (x is None and y is None) or same_bits(down(x), down(y)), f"{entry} {arena.name}: differs from the coupled entry point"
            count += 1
    # ... and the segmented forms: both three-segment layouts and the 35 segments with every segment on that hyper set
    arenas = [R.Arena(f"{name}_wd0", n, [(b, e, h) for b, e in R.three_segments(lengths, n)], 1.0, seed=860 + i)
              for i, (name, (lengths, n)) in enumerate(sorted(R.THREE_LAYOUTS.items()))]
    bounds, n = R.thirty_five_bounds()
    arenas.append(R.Arena("thirty_five_wd0", n, [(b, e, h) for b, e in bounds], 1.0, seed=863))
    for arena in arenas:
        for entry in (HOST_EX, DEV_EX):
            for mode in (None, "norm"):
                clip4, _ = record_for(arena, mode)
                a, b = run_ex(entry, arena, [1] * len(arena.segs), clip4), run_coupled(entry, arena, clip4)
                for x, y in zip(a, b):
                    assert (x is None and y is None) or same_bits(down(x), down(y)), f"{entry} {case_of(arena, mode)}: differs from coupled"
                count += 1
    print(f"ADAMW-FORMS wd = 0: {count} comparisons, decoupled and coupled entry points agree in every bit")


# ---------------------------------------------------------------- twenty teacher-forced steps
def test_twenty_teacher_forced_steps_of_adamw_step():
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
        ops.adamw_step(p, up(arena.g), m, v, lr, b1, b2, eps, wd, step)
        refs = W.references(arena, state=before, lrs=[(lr, step)])
        hold(fails, "adamw_step", f"sequence_n4100_step{step:02d}", arena, refs, (down(p), down(m), down(v)), p_before=before[0])
    fails.done()


def test_twenty_teacher_forced_steps_of_adam_step_segments_dev_ex():
    arena = R.sequence_arena()
    p, _, m, v = tensors(arena)
    state = rows_before([1] * len(arena.segs))
    table = np.array(R.lr_table(), dtype=np.float32)
    modes = [1] * len(arena.segs)
    fails = Failures()
    for step in range(1, 21):
        lrs = []
        for b, e, h in arena.segs:
            arena.g[b:e] = R.sequence_gradient(e - b, step, seed=820 + h)
            table[R.lr_index(h)] = R.sequence_lr(HYPER[h][0], step + h)            # the host rewrites the table between steps
            lrs.append((float(table[R.lr_index(h)]), step))
        before = (down(p).copy(), down(m).copy(), down(v).copy())
        ops.adam_step_segments_dev_ex(p, up(arena.g), m, v, dev_records(arena, modes), up(table), state)
        case = f"sequence_n4100_step{step:02d}"
        hold(fails, DEV_EX, case, arena, W.references(arena, state=before, lrs=lrs), (down(p), down(m), down(v)), p_before=before[0])
        hold_rows(fails, "adam_tick_segments", case, state, [(step, HYPER[h][1], HYPER[h][2]) for _, _, h in arena.segs])
        mask = arena.outside()
        for got, old in zip((p, m, v), (arena.p, arena.m, arena.v)):
            fails.check(same_bits(down(got)[mask], old[mask]), f"{case}: something outside the segments changed")
    fails.done()


# ---------------------------------------------------------------- the version counters, every wrapper
WRAPPERS = ["adam_step", "adamw_step", "adam_step_dev", "adamw_step_dev", "adam_step_segments", "adam_step_segments_clip",
            "adam_step_segments_ex", "adam_step_segments_dev", "adam_step_segments_dev_clip", "adam_step_segments_dev_ex"]


@pytest.mark.parametrize("entry", WRAPPERS)
def test_every_wrapper_bumps_the_version_counters_of_what_the_kernel_wrote(entry):
    """The kernels write param, exp_avg and exp_avg_sq through raw pointers; autograd's saved-tensor checks and the inference
    path's cache of split weights learn of it from the version counters alone, so every ops wrapper must raise all three."""
    lr, b1, b2, eps, wd = 1e-3, 0.9, 0.999, 1e-8, 1e-2
    p, g, m, v = (torch.full((64,), x, device=dev()) for x in (0.5, 0.25, 0.0, 0.0))
    before = [t._version for t in (p, m, v)]
    segmented, on_dev, ex = "segments" in entry, "_dev" in entry, entry.endswith("_ex")
    bounds = [(0, 16), (32, 48)]
    args = []
    if segmented:
        args.append([(b, e) + ((0, b1, b2, eps, wd) if on_dev else (lr, b1, b2, eps, wd, 1)) + ((k,) if ex else ()) for k, (b, e) in enumerate(bounds)])
    if on_dev:
        args += [up(np.array([lr], dtype=np.float32)), torch.zeros((2, 3) if segmented else (3,), device=dev())]
    if not segmented:
        args += [b1, b2, eps, wd] if on_dev else [lr, b1, b2, eps, wd, 1]
    if ex or entry.endswith("_clip"):
        args.append(up(np.array([0.0, 1.0, 0.0, 0.0], dtype=np.float32)))
    getattr(ops, entry)(p, g, m, v, *args)
    torch.cuda.synchronize()
    assert all(t._version > was for t, was in zip((p, m, v), before)), (entry, before, [t._version for t in (p, m, v)])
    assert bool((p != 0.5).any()) and bool((m != 0).any())              # (the call did run its update)
