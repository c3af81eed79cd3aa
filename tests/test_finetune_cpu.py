"""Fine-tuning without a GPU: the C ABI of the segmented Adam step (header, binding and built library agree), the segment
planner over arena layouts, and the optimizer's construction / checkpoint surface for parameter groups.

The segments travel through the C ABI as three parallel HOST arrays (bounds, hyper-parameters, step counts) and become a
by-value kernel argument inside the library; the header therefore declares a function and a constant and no new struct."""
import ctypes as C

import pytest
import torch

import cabi_header as hdr
import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd import _lib
from rot_mvgaze_amd.optim import Adam, Segment, plan_segments


# ---------------------------------------------------------------- C ABI
def test_segmented_step_is_declared_bound_and_exported():
    import __graft_entry__ as ge
    ge.build()
    lib = _lib.lib()
    ret, params = hdr.functions["mvg_adam_step_segments"]
    assert ret == "int"
    assert params == [("float*", "param"), ("float*", "grad"), ("float*", "exp_avg"), ("float*", "exp_avg_sq"), ("int64_t", "n"),
                      ("int64_t*", "host_bounds"), ("float*", "host_hyper"), ("int32_t*", "host_steps"), ("int", "n_segments"),
                      ("void*", "stream")]
    res, args = _lib.SIGNATURES["mvg_adam_step_segments"]
    assert res is C.c_int and len(args) == len(params)
    assert args[4] is C.c_int64 and args[8] is C.c_int and all(a is C.c_void_p for a in args[:4] + [args[9]])
    assert [a._type_ for a in args[5:8]] == [C.c_int64, C.c_float, C.c_int32]
    assert hasattr(lib, "mvg_adam_step_segments")
    assert hdr.constants["MVG_ADAM_MAX_SEGMENTS"] == _lib.ADAM_MAX_SEGMENTS == 16
    # additive: the version every earlier entry point was built against
    assert hdr.constants["MVG_ABI_VERSION"] == _lib.ABI_VERSION == lib.mvg_abi_version() == 13
    # the neighbours it was added to are what they were
    assert hdr.arity("mvg_adam_step") == 12 and hdr.arity("mvg_adam_step_dev") == 12


# ---------------------------------------------------------------- plan_segments
# a small arena in the model's order: head (with 2-element biases), lifter, then the backbone from its last block to the stem
LAYOUT = [("head.w0", 4096), ("head.b0", 64), ("head.w1", 128), ("head.b1", 2), ("fuser.w", 1000), ("fuser.b", 10),
          ("lifter.w", 2048), ("lifter.b", 6),
          ("layer4.conv", 9 * 64), ("layer4.bn.w", 8), ("layer4.bn.b", 8), ("layer3.conv", 9 * 32), ("layer3.bn.w", 4),
          ("layer3.bn.b", 4), ("stem.conv", 147 * 8), ("stem.bn.w", 8), ("stem.bn.b", 8)]


def _entries():
    out, off = [], 0
    for _, n in LAYOUT:
        out.append((off, n))
        off += (n + 3) // 4 * 4
    return out, off


def _idx(prefix):
    return [i for i, (name, _) in enumerate(LAYOUT) if name.startswith(prefix)]


def _aligned(segs, total):
    for s in segs:
        assert s.begin % 4 == 0 and s.end % 4 == 0 and 0 <= s.begin < s.end <= total
    for a, b in zip(segs, segs[1:]):
        assert a.end <= b.begin


def test_plan_one_group_all_gradients_is_one_segment():
    e, total = _entries()
    segs = plan_segments(e, ["g"] * len(e), [True] * len(e), [3] * len(e))
    assert segs == [Segment(0, total, "g", 3)]


def test_plan_head_and_backbone_groups_meet_at_the_border():
    e, total = _entries()
    first_bb = _idx("layer4")[0]
    groups = ["head" if i < first_bb else "bb" for i in range(len(e))]
    segs = plan_segments(e, groups, [True] * len(e), [1] * len(e))
    border = e[first_bb][0]
    assert segs == [Segment(0, border, "head", 1), Segment(border, total, "bb", 1)]
    _aligned(segs, total)


def test_plan_frozen_prefix_stops_before_it():
    """The network's first stages sit at the END of the arena (grad-ready order): the segment ends where they begin."""
    e, total = _entries()
    frozen = set(_idx("stem") + _idx("layer3"))
    has = [i not in frozen for i in range(len(e))]
    segs = plan_segments(e, ["g"] * len(e), has, [1] * len(e))
    assert segs == [Segment(0, e[_idx("layer3")[0]][0], "g", 1)]


def test_plan_hole_in_the_middle_gives_two_segments():
    e, total = _entries()
    hole = _idx("lifter")
    has = [i not in hole for i in range(len(e))]
    segs = plan_segments(e, ["g"] * len(e), has, [2] * len(e))
    assert segs == [Segment(0, e[hole[0]][0], "g", 2), Segment(e[hole[-1] + 1][0], total, "g", 2)]
    _aligned(segs, total)


def test_plan_step_counts_split_a_run():
    e, total = _entries()
    first_bb = _idx("layer4")[0]
    steps = [5 if i < first_bb else 1 for i in range(len(e))]          # the backbone was unfrozen four steps later
    segs = plan_segments(e, ["g"] * len(e), [True] * len(e), steps)
    assert segs == [Segment(0, e[first_bb][0], "g", 5), Segment(e[first_bb][0], total, "g", 1)]


def test_plan_two_element_biases_keep_bounds_on_slots():
    e, total = _entries()
    b1 = _idx("head.b1")[0]
    assert LAYOUT[b1][1] == 2
    # only the 2-element bias takes part: its segment is its whole 4-element slot
    segs = plan_segments(e, ["g"] * len(e), [i == b1 for i in range(len(e))], [1] * len(e))
    assert segs == [Segment(e[b1][0], e[b1][0] + 4, "g", 1)]
    # everything but it: the run before ends on a slot boundary, the run behind starts on one
    segs = plan_segments(e, ["g"] * len(e), [i != b1 for i in range(len(e))], [1] * len(e))
    assert segs == [Segment(0, e[b1][0], "g", 1), Segment(e[b1][0] + 4, total, "g", 1)]
    # and padded entries inside a run (the 6- and 10-element biases) do not split it
    _aligned(plan_segments(e, ["g"] * len(e), [True] * len(e), [1] * len(e)), total)


def test_plan_no_gradients_no_segment():
    e, _ = _entries()
    assert plan_segments(e, ["g"] * len(e), [False] * len(e), [0] * len(e)) == []
    assert plan_segments([], [], [], []) == []


def test_plan_rejects_what_it_cannot_place():
    with pytest.raises(ValueError):
        plan_segments([(0, 4), (2, 4)], ["g", "g"], [True, True], [1, 1])        # unaligned / overlapping entries
    with pytest.raises(ValueError):
        plan_segments([(0, 4)], ["g"], [True], [0])                              # taking part with step 0
    with pytest.raises(ValueError):
        plan_segments([(0, 4)], ["g", "g"], [True], [1])


# ---------------------------------------------------------------- optim.Adam: groups and checkpoints
def _model():
    from rot_mvgaze_amd.model import FeatRotationSymm
    return FeatRotationSymm(backbone_depth=18, num_iter=3)


def _two_groups(m):
    bb = [p for n, p in m.named_parameters() if n.startswith("_feat_extractor")]
    head = [p for n, p in m.named_parameters() if not n.startswith("_feat_extractor")]
    return [{"params": bb, "lr": 1e-4, "weight_decay": 1e-6}, {"params": head, "lr": 1e-3, "weight_decay": 0.0}]


def test_adam_takes_parameter_groups():
    m = _model()
    opt = Adam(_two_groups(m), lr=5e-4, betas=(0.8, 0.99))
    assert [g["lr"] for g in opt.param_groups] == [1e-4, 1e-3]
    assert [g["weight_decay"] for g in opt.param_groups] == [1e-6, 0.0]
    assert all(g["betas"] == (0.8, 0.99) and g["eps"] == 1e-8 for g in opt.param_groups)
    assert len(opt._owners()) == 1                                  # both groups lead to the one model
    sched = torch.optim.lr_scheduler.CyclicLR(opt, base_lr=[1e-6, 1e-5], max_lr=[1e-4, 1e-3], step_size_up=2, cycle_momentum=False)
    assert [g["lr"] for g in opt.param_groups] == [1e-6, 1e-5]      # the scheduler drives each group
    del sched
    with pytest.raises(ValueError):
        Adam([{"params": list(m.parameters()), "lr": -1.0}])


def test_capturable_with_two_groups_is_refused_at_construction():
    m = _model()
    with pytest.raises(NotImplementedError, match="one parameter group.*at construction"):
        Adam(_two_groups(m), capturable=True)
    Adam(m.parameters(), capturable=True)                           # one group: as before


def test_old_single_step_arena_state_loads():
    """An mvg_arena_state entry written before per-parameter step counts: every parameter gets its one "step"."""
    m = _model()
    opt = Adam(m.parameters(), lr=1e-3)
    sd = opt.state_dict()
    assert sd["mvg_arena_state"] == []
    n = 64
    sd["mvg_arena_state"] = [{"step": 7, "exp_avg": torch.full((n,), 0.5), "exp_avg_sq": torch.full((n,), 0.25)}]
    opt2 = Adam(m.parameters(), lr=1e-3)
    opt2.load_state_dict(sd)
    st = opt2._state_for(m, torch.zeros(n), 5)                       # what the next step() adopts for a 5-parameter arena
    assert st["steps"] == [7] * 5 and st["step"] == 7
    assert torch.equal(st["exp_avg"], torch.full((n,), 0.5)) and torch.equal(st["exp_avg_sq"], torch.full((n,), 0.25))
    # today's format carries the counts themselves
    sd["mvg_arena_state"] = [{"step": 7, "steps": [7, 7, 0, 2, 7], "exp_avg": torch.zeros(n), "exp_avg_sq": torch.zeros(n)}]
    opt3 = Adam(m.parameters(), lr=1e-3)
    opt3.load_state_dict(sd)
    assert opt3._state_for(m, torch.zeros(n), 5)["steps"] == [7, 7, 0, 2, 7]
