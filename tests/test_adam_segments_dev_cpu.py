"""The device-resident segmented Adam step without a GPU: the C ABI of mvg_adam_step_segments_dev (header and binding agree type for
type, the ABI version and the neighbours' arities are what they were), the construction surface of optim.Adam(capturable="segments")
and the plan signature, which is host-only: equal for equal plans, different after a requires_grad flip or a betas change, and blind
to the learning rate (that lives in the device vector, not in the plan)."""
import ctypes as C

import pytest

import cabi_header as hdr
import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd import _lib
from rot_mvgaze_amd.optim import Adam

CTYPE = {"float*": C.c_void_p, "void*": C.c_void_p, "int64_t": C.c_int64, "int": C.c_int}
HOST_ARRAYS = {"host_bounds": C.c_int64, "host_hyper": C.c_float, "host_lr_index": C.c_int32}


# ---------------------------------------------------------------- C ABI
def test_header_signature_matches_the_binding_type_for_type():
    ret, params = hdr.functions["mvg_adam_step_segments_dev"]
    assert ret == "int"
    assert params == [("float*", "param"), ("float*", "grad"), ("float*", "exp_avg"), ("float*", "exp_avg_sq"), ("int64_t", "n"),
                      ("int64_t*", "host_bounds"), ("float*", "host_hyper"), ("int32_t*", "host_lr_index"), ("int", "n_segments"),
                      ("float*", "lr_dev"), ("int", "n_lr"), ("float*", "state3_dev"), ("void*", "stream")]
    res, args = _lib.SIGNATURES["mvg_adam_step_segments_dev"]
    assert res is C.c_int and len(args) == len(params)
    for (ctype, name), arg in zip(params, args):
        if name in HOST_ARRAYS:                      # host arrays are typed pointers, device buffers and the stream are void *
            assert arg._type_ is HOST_ARRAYS[name], name
        else:
            assert arg is CTYPE[ctype], name


def test_abi_version_and_the_neighbours_are_unchanged():
    assert hdr.constants["MVG_ABI_VERSION"] == _lib.ABI_VERSION == 13
    assert hdr.constants["MVG_ADAM_MAX_SEGMENTS"] == _lib.ADAM_MAX_SEGMENTS == 16
    assert hdr.arity("mvg_adam_step") == 12 and hdr.arity("mvg_adam_step_dev") == 12 and hdr.arity("mvg_adam_step_segments") == 10
    for name, n in (("mvg_adam_step", 12), ("mvg_adam_step_dev", 12), ("mvg_adam_step_segments", 10)):
        assert len(_lib.SIGNATURES[name][1]) == n


def test_built_library_exports_the_entry_point():
    import __graft_entry__ as ge
    ge.build()
    lib = _lib.lib()
    assert hasattr(lib, "mvg_adam_step_segments_dev") and lib.mvg_abi_version() == 13


# ---------------------------------------------------------------- optim.Adam(capturable="segments")
def _model():
    from rot_mvgaze_amd.model import FeatRotationSymm
    return FeatRotationSymm(backbone_depth=18, num_iter=3)


def _two_groups(m):
    bb = [p for n, p in m.named_parameters() if n.startswith("_feat_extractor")]
    head = [p for n, p in m.named_parameters() if not n.startswith("_feat_extractor")]
    return [{"params": head, "lr": 1e-3, "weight_decay": 0.0}, {"params": bb, "lr": 1e-4, "weight_decay": 1e-6}]


def _entries(m):
    """An arena layout over the CPU model: every parameter on a 4-element slot, head first (the order the model itself uses needs a
    device; any fixed order serves the planner)."""
    named = list(m.named_parameters())
    order = [p for n, p in named if not n.startswith("_feat_extractor")] + [p for n, p in named if n.startswith("_feat_extractor")]
    out, off = [], 0
    for p in order:
        out.append((p, off, p.numel()))
        off += (p.numel() + 3) // 4 * 4
    return out


def test_segments_mode_takes_parameter_groups_on_the_cpu():
    m = _model()
    opt = Adam(_two_groups(m), capturable="segments")
    assert opt.capturable == "segments" and bool(opt.capturable)          # truthy: GraphedStep accepts it
    assert len(opt.param_groups) == 2
    assert Adam(m.parameters(), capturable=True).capturable is True and Adam(m.parameters()).capturable is False
    with pytest.raises(NotImplementedError, match="one parameter group.*at construction"):
        Adam(_two_groups(m), capturable=True)                             # True keeps its pinned refusal


def test_any_other_capturable_value_is_refused():
    m = _model()
    with pytest.raises(ValueError, match="capturable"):
        Adam(m.parameters(), capturable="bogus")
    with pytest.raises(ValueError, match="capturable"):
        Adam(_two_groups(m), capturable="Segments")


def test_plan_signature_is_host_only_and_sees_what_a_captured_plan_holds():
    m = _model()
    ents = _entries(m)
    opt = Adam(_two_groups(m), capturable="segments")
    sig = opt.plan_signature(ents)                                        # CPU parameters: no device, no library call
    (segs,) = sig
    total = ents[-1][1] + (ents[-1][2] + 3) // 4 * 4
    border = next(off for (p, off, _) in ents if any(p is q for q in opt.param_groups[1]["params"]))
    assert segs == ((0, border, 0, 0.9, 0.999, 1e-8, 0.0), (border, total, 1, 0.9, 0.999, 1e-8, 1e-6))
    # equal plans, equal signatures: a second optimizer over the same groups
    assert Adam(_two_groups(m), capturable="segments").plan_signature(ents) == sig
    # the learning rate is not part of it
    opt.param_groups[0]["lr"] = 0.5
    opt.param_groups[1]["lr"] = 0.25
    assert opt.plan_signature(ents) == sig
    # a requires_grad flip is
    p = ents[3][0]
    p.requires_grad_(False)
    flipped = opt.plan_signature(ents)
    assert flipped != sig and len(flipped[0]) == 3                        # the hole splits the head's segment
    p.requires_grad_(True)
    assert opt.plan_signature(ents) == sig
    # ... and so is a betas change
    opt.param_groups[1]["betas"] = (0.8, 0.999)
    assert opt.plan_signature(ents) != sig
    opt.param_groups[1]["betas"] = (0.9, 0.999)
    assert opt.plan_signature(ents) == sig
    # two groups with the same constants stay two segments (equal learning rates today may differ tomorrow)
    same = Adam([{"params": g["params"]} for g in _two_groups(m)], capturable="segments")
    assert [s[2] for s in same.plan_signature(ents)[0]] == [0, 1]
