"""mvg_adam_step_segments_dev at kernel level: the segmented Adam step with its learning rates (one float per parameter group) and
its step counters / bias corrections (one row per segment) on the device.

Reference for every slice: ops.adam_step_dev (mvg_adam_step_dev) on clones of that slice, with a one-element lr_dev and a one-row
state3 holding the same starting count.  Both run the same device arithmetic (adam_tick1, adam_elem / adam_slot), so the bar is
torch.equal - on the parameter, both moments and the state rows.  Outside the segments the int32 views are unchanged.  Shapes are
the ones tests/test_finetune_gpu.py found necessary for mvg_adam_step_segments."""
import numpy as np
import pytest
import torch

import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd import ops

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def _arena(n, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g).to(dev())
    gr = (torch.randn(n, generator=g) * 0.1).to(dev())
    m = (torch.randn(n, generator=g) * 0.01).to(dev())
    v = (torch.rand(n, generator=g) * 1e-3).to(dev())
    return p, gr, m, v


def _rows(counts):
    return torch.tensor([[float(c), 0.0, 0.0] for c in counts], dtype=torch.float32).reshape(-1, 3).to(dev())


def _check(n, segs, lrs, counts, seed=0, calls=1, lrs_second=None):
    """segs: (begin, end, lr_index, b1, b2, eps, wd).  Runs ``calls`` steps of the segmented device step over one arena and of
    adam_step_dev over clones of each slice; compares slices, state rows and everything outside the segments."""
    p, g, m, v = _arena(n, seed)
    before = [t.clone() for t in (p, m, v)]
    lr_dev = torch.tensor(lrs, dtype=torch.float32).to(dev())
    state = _rows(counts)
    ref = []
    for (b, e, li, *_), c in zip(segs, counts):
        ref.append([t[b:e].clone() for t in (p, g, m, v)] + [torch.tensor([lrs[li]], dtype=torch.float32).to(dev()), _rows([c]).reshape(3)])
    for call in range(calls):
        if call == 1 and lrs_second is not None:                                     # the host rewrites an entry between two steps
            lr_dev.copy_(torch.tensor(lrs_second, dtype=torch.float32))
            for (b, e, li, *_), r in zip(segs, ref):
                r[4].fill_(lrs_second[li])
        for (b, e, li, b1, b2, eps, wd), r in zip(segs, ref):
            ops.adam_step_dev(r[0], r[1], r[2], r[3], r[4], r[5], b1, b2, eps, wd)
        ops.adam_step_segments_dev(p, g, m, v, segs, lr_dev, state)
    torch.cuda.synchronize()
    outside = torch.ones(n, dtype=torch.bool, device=dev())
    for k, ((b, e, *_), r, c) in enumerate(zip(segs, ref, counts)):
        outside[b:e] = False
        for got, want, what in zip((p, m, v), (r[0], r[2], r[3]), ("param", "exp_avg", "exp_avg_sq")):
            assert torch.equal(got[b:e], want), f"{what} of segment {k} [{b}, {e})"
        assert not torch.equal(p[b:e], before[0][b:e])                               # (the step did move the slice)
        assert torch.equal(state[k], r[5]), f"state row {k}: {state[k].tolist()} vs {r[5].tolist()}"
        assert float(state[k, 0].item()) == c + calls, f"row {k} advanced {state[k, 0].item() - c} times in {calls} call(s)"
    for got, old, what in zip((p, m, v), before, ("param", "exp_avg", "exp_avg_sq")):
        assert torch.equal(got[outside].view(torch.int32), old[outside].view(torch.int32)), f"{what} outside the segments"


THREE = [(0, 4, 1, 0.9, 0.999, 1e-8, 0.0),                    # a 4-element segment starting at 0
         (64, 1028, 0, 0.8, 0.99, 1e-6, 1e-6),                # ... a hole before and behind this one
         (2048, 4096, 1, 0.5, 0.9, 1e-3, 1e-2)]               # ... and one ending at n; it shares lr entry 1 with the first


def test_three_segments_with_holes_their_own_constants_and_counts():
    _check(4096, THREE, lrs=[1e-4, 5e-2], counts=[0, 4, 99])


def _random_segments(seed=3):
    rng = np.random.default_rng(seed)
    segs, counts, off = [], [], 0
    for i in range(35):                                                              # 16 + 16 + 3: three chunks
        off += 4 * int(rng.integers(0, 5))                                           # holes of 0 .. 16 elements
        ln = 4 * int(rng.integers(1, 17))                                            # 4 .. 64 elements
        segs.append((off, off + ln, int(rng.integers(0, 5)), float(rng.uniform(0.5, 0.95)), float(rng.uniform(0.9, 0.9999)), 1e-8,
                     float(rng.choice([0.0, 1e-6, 1e-2]))))
        counts.append(int(rng.integers(0, 50)))
        off += ln
    assert len(segs) == 35 and min(e - b for b, e, *_ in segs) >= 4 and max(e - b for b, e, *_ in segs) <= 64
    assert len({s[2] for s in segs}) == 5 and min(counts) >= 0 and max(counts) <= 49
    return segs, counts, off + 64


def test_more_segments_than_one_launch_takes():
    segs, counts, n = _random_segments()
    lrs = [1e-5, 1e-4, 1e-3, 3e-3, 1e-2]
    _check(n, segs, lrs, counts)


def test_grid_stride_loop_over_the_concatenated_length():
    cap = 8192 * 256 * 4                                                             # the grid cap times 4 elements per lane
    a = 5_000_000
    segs = [(1024, 1024 + a, 0, 0.9, 0.999, 1e-8, 1e-6),
            (1024 + a + 4096, 1024 + a + 4096 + (cap - a) + 512, 1, 0.8, 0.99, 1e-8, 0.0)]
    assert sum(e - b for b, e, *_ in segs) == cap + 512
    _check(segs[-1][1] + 2048, segs, lrs=[1e-3, 1e-4], counts=[1, 6])


def test_two_calls_advance_every_row_twice_and_honour_a_rewritten_lr():
    # the second call runs with the step-2 (count + 2) corrections: the per-slice reference ticks twice as well, and its rows are
    # compared bit for bit; lr entry 1 (two segments read it) is rewritten between the calls, entry 0 is not
    _check(4096, THREE, lrs=[1e-4, 5e-2], counts=[0, 4, 99], calls=2, lrs_second=[1e-4, 2e-3])
    segs, counts, n = _random_segments(5)
    _check(n, segs, [1e-5, 1e-4, 1e-3, 3e-3, 1e-2], counts, calls=2, lrs_second=[2e-5, 1e-4, 5e-4, 3e-3, 2e-2])


def test_a_rewritten_lr_changes_the_second_step():
    """(the comparison above would also hold if both sides ignored the rewrite: the second step must differ from an unrewritten one)"""
    out = []
    for second in ([1e-4, 5e-2], [1e-4, 2e-3]):
        p, g, m, v = _arena(4096, 0)
        lr_dev = torch.tensor([1e-4, 5e-2], dtype=torch.float32).to(dev())
        state = _rows([0, 4, 99])
        ops.adam_step_segments_dev(p, g, m, v, THREE, lr_dev, state)
        lr_dev.copy_(torch.tensor(second, dtype=torch.float32))
        ops.adam_step_segments_dev(p, g, m, v, THREE, lr_dev, state)
        out.append(p)
    assert torch.equal(out[0][64:1028], out[1][64:1028])                             # reads entry 0
    assert not torch.equal(out[0][0:4], out[1][0:4]) and not torch.equal(out[0][2048:], out[1][2048:])


GOOD = (0, 64, 0)


@pytest.mark.parametrize("name,segs,null", [
    ("unsorted", [(64, 128, 0), (0, 32, 0)], None),
    ("overlap", [(0, 64, 0), (32, 96, 0)], None),
    ("aligned", [GOOD, (130, 194, 0)], None),
    ("outside", [GOOD, (4000, 4100, 0)], None),
    ("empty", [GOOD, (128, 128, 0)], None),
    ("lr index", [GOOD, (128, 256, 2)], None),
    ("lr index", [GOOD, (128, 256, -1)], None),
    ("null", [GOOD, (128, 256, 1)], "lr_dev"),
    ("null", [GOOD, (128, 256, 1)], "state3"),
    ("null", [GOOD, (128, 256, 1)], "grad"),
], ids=["unsorted", "overlap", "aligned", "outside", "empty", "lr_index_high", "lr_index_negative", "null_lr_dev", "null_state3", "null_grad"])
def test_bad_calls_are_rejected_before_any_launch(name, segs, null):
    n = 4096
    p, g, m, v = _arena(n, 2)
    lr_dev = torch.tensor([1e-3, 1e-2], dtype=torch.float32).to(dev())
    state = _rows([3] * len(segs))
    before = [t.clone() for t in (p, m, v, state)]
    args = {"grad": g, "lr_dev": lr_dev, "state3": state}
    if null:
        args[null] = None
    with pytest.raises(RuntimeError, match="adam_step_segments_dev: .*" + name):
        ops.adam_step_segments_dev(p, args["grad"], m, v, [(b, e, li, 0.9, 0.999, 1e-8, 0.0) for b, e, li in segs], args["lr_dev"], args["state3"])
    torch.cuda.synchronize()
    for got, old in zip((p, m, v, state), before):                                   # neither the valid first segment nor the tick ran
        assert torch.equal(got.view(torch.int32), old.view(torch.int32))
