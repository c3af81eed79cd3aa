"""Global-norm gradient clipping and the non-finite guard without a GPU: the float64 reference of tests/grad_clip_ref.py pinned
to torch.nn.utils.clip_grad_norm_, the C ABI of the four new entry points (header and binding agree type for type, the version and
the existing Adam entry points are what they were, the built library exports the symbols) and the construction surface of
optim.Adam(max_grad_norm=, skip_nonfinite=)."""
import ctypes as C
import math

import pytest
import torch

import cabi_header as hdr
import grad_clip_ref as ref
import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd import _lib
from rot_mvgaze_amd.optim import Adam

CTYPE = {"float*": C.c_void_p, "void*": C.c_void_p, "int64_t": C.c_int64, "int": C.c_int, "float": C.c_float}
HOST_ARRAYS = {"host_bounds": C.c_int64, "host_hyper": C.c_float, "host_steps": C.c_int32, "host_lr_index": C.c_int32}


# ---------------------------------------------------------------- the reference against torch
def _tensors(seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, generator=g, dtype=torch.float64) * scale) for n in (4, 964, 2048)]


def _arena_of(grads):
    """The gradients laid into one arena with holes between them (poisoned: the reference must not read them)."""
    begins, off = [], 0
    for t in grads:
        off += 60
        begins.append(off)
        off += t.numel()
    arena = torch.full((off + 32,), 1e30, dtype=torch.float64)
    for b, t in zip(begins, grads):
        arena[b:b + t.numel()] = t
    return arena, [(b, b + t.numel()) for b, t in zip(begins, grads)]


@pytest.mark.parametrize("max_norm,binds", [(1.0, True), (1e9, False)], ids=["binds", "does_not_bind"])
def test_reference_is_clip_grad_norm(max_norm, binds):
    grads = _tensors(0)
    arena, bounds = _arena_of(grads)
    r = ref.reference(arena, bounds, max_norm, skip_nonfinite=False)
    params = [torch.nn.Parameter(torch.zeros_like(t)) for t in grads]
    for p, t in zip(params, grads):
        p.grad = t.clone()
    total = torch.nn.utils.clip_grad_norm_(params, max_norm)
    assert abs(float(total) - r["norm"]) <= 1e-12 * r["norm"]
    assert (r["coef"] < 1.0) == binds and not r["skipped"]
    if not binds:
        assert r["coef"] == 1.0
    for p, t in zip(params, grads):
        want = t * r["coef"]
        assert float((p.grad - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_reference_with_a_nan_gradient_is_torch_with_error_if_nonfinite_false():
    grads = _tensors(1)
    grads[1][17] = float("nan")
    arena, bounds = _arena_of(grads)
    r = ref.reference(arena, bounds, 1.0, skip_nonfinite=False)
    params = [torch.nn.Parameter(torch.zeros_like(t)) for t in grads]
    for p, t in zip(params, grads):
        p.grad = t.clone()
    total = torch.nn.utils.clip_grad_norm_(params, 1.0, error_if_nonfinite=False)
    assert math.isnan(float(total)) and math.isnan(r["norm"]) and math.isnan(r["coef"]) and not r["skipped"]
    assert all(bool(torch.isnan(p.grad).all()) for p in params)                  # torch turns every gradient NaN: coef is NaN
    # the guard's decision on the same data, and on an inf; a clean gradient is not skipped; no clipping: coef 1
    guarded = ref.reference(arena, bounds, 1.0, skip_nonfinite=True)
    assert guarded["skipped"] and guarded["coef"] == 0.0
    grads[1][17] = float("inf")
    arena, bounds = _arena_of(grads)
    r = ref.reference(arena, bounds, 1.0, skip_nonfinite=False)
    assert r["norm"] == float("inf") and r["coef"] == 0.0                          # torch: max_norm / inf
    assert ref.reference(arena, bounds, 1.0, skip_nonfinite=True)["skipped"]
    arena, bounds = _arena_of(_tensors(2))
    assert not ref.reference(arena, bounds, None, skip_nonfinite=True)["skipped"]
    assert ref.reference(arena, bounds, None, skip_nonfinite=True)["coef"] == 1.0


def test_one_ulp_helper():
    import numpy as np
    x = np.float32(1.5)
    assert ref.within_one_ulp(x, x) and ref.within_one_ulp(np.nextafter(x, np.float32(2)), x)
    assert not ref.within_one_ulp(np.nextafter(np.nextafter(x, np.float32(2)), np.float32(2)), x)
    assert ref.within_one_ulp(float("nan"), np.float32("nan")) and not ref.within_one_ulp(1.0, np.float32("nan"))


# ---------------------------------------------------------------- C ABI
NEW = {
    "mvg_grad_norm_workspace_bytes": ("int64_t", [("int", "n_segments")]),
    "mvg_grad_norm_segments": ("int", [("float*", "grad"), ("int64_t", "n"), ("int64_t*", "host_bounds"), ("int", "n_segments"),
                                       ("float", "max_norm"), ("int", "skip_nonfinite"), ("void*", "ws"), ("int64_t", "ws_bytes"),
                                       ("float*", "clip4_dev"), ("void*", "stream")]),
    "mvg_adam_step_segments_clip": ("int", [("float*", "param"), ("float*", "grad"), ("float*", "exp_avg"), ("float*", "exp_avg_sq"),
                                            ("int64_t", "n"), ("int64_t*", "host_bounds"), ("float*", "host_hyper"),
                                            ("int32_t*", "host_steps"), ("int", "n_segments"), ("float*", "clip4_dev"), ("void*", "stream")]),
    "mvg_adam_step_segments_dev_clip": ("int", [("float*", "param"), ("float*", "grad"), ("float*", "exp_avg"), ("float*", "exp_avg_sq"),
                                                ("int64_t", "n"), ("int64_t*", "host_bounds"), ("float*", "host_hyper"),
                                                ("int32_t*", "host_lr_index"), ("int", "n_segments"), ("float*", "lr_dev"), ("int", "n_lr"),
                                                ("float*", "state3_dev"), ("float*", "clip4_dev"), ("void*", "stream")]),
}


@pytest.mark.parametrize("name", sorted(NEW))
def test_header_signature_matches_the_binding_type_for_type(name):
    ret, params = hdr.functions[name]
    assert (ret, params) == NEW[name]
    res, args = _lib.SIGNATURES[name]
    assert res is CTYPE[ret] and len(args) == len(params)
    for (ctype, pname), arg in zip(params, args):
        if pname in HOST_ARRAYS:                     # host arrays are typed pointers, device buffers and the stream are void *
            assert arg._type_ is HOST_ARRAYS[pname], pname
        else:
            assert arg is CTYPE[ctype], pname


def test_the_clipped_steps_take_their_neighbours_arguments_and_the_record():
    for base in ("mvg_adam_step_segments", "mvg_adam_step_segments_dev"):
        a, b = hdr.functions[base][1], hdr.functions[base + "_clip"][1]
        assert b == a[:-1] + [("float*", "clip4_dev")] + a[-1:]


def test_abi_version_and_the_existing_adam_entry_points_are_unchanged():
    assert hdr.constants["MVG_ABI_VERSION"] == _lib.ABI_VERSION == 13
    assert hdr.constants["MVG_ADAM_MAX_SEGMENTS"] == _lib.ADAM_MAX_SEGMENTS == 16
    for name, n in (("mvg_adam_step", 12), ("mvg_adam_step_dev", 12), ("mvg_adam_step_segments", 10), ("mvg_adam_step_segments_dev", 13)):
        assert hdr.arity(name) == n == len(_lib.SIGNATURES[name][1]), name


def test_built_library_exports_the_entry_points():
    import __graft_entry__ as ge
    ge.build()
    lib = _lib.lib()
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.mvg_abi_version() == 13


# ---------------------------------------------------------------- optim.Adam(max_grad_norm=, skip_nonfinite=)
def _model():
    from rot_mvgaze_amd.model import FeatRotationSymm
    return FeatRotationSymm(backbone_depth=18, num_iter=3)


def test_constructor_surface():
    m = _model()
    opt = Adam(m.parameters())
    assert opt.max_grad_norm is None and opt.skip_nonfinite is False
    opt = Adam(m.parameters(), max_grad_norm=2, skip_nonfinite=True, capturable="segments")
    assert opt.max_grad_norm == 2.0 and opt.skip_nonfinite is True
    for bad in (0, -1, 0.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            Adam(m.parameters(), max_grad_norm=bad)
    with pytest.raises(ValueError, match="segments"):
        Adam(m.parameters(), capturable=True, max_grad_norm=1.0)
    with pytest.raises(ValueError, match="segments"):
        Adam(m.parameters(), capturable=True, skip_nonfinite=True)
    assert Adam(m.parameters(), capturable=True).capturable is True              # ... and alone it is what it was


def test_the_settings_are_not_in_the_groups_or_the_state_dict():
    m = _model()
    plain, clipped = Adam(m.parameters()), Adam(m.parameters(), max_grad_norm=1.0, skip_nonfinite=True)
    a, b = plain.state_dict(), clipped.state_dict()
    assert set(a) == set(b) and [set(g) for g in a["param_groups"]] == [set(g) for g in b["param_groups"]]
    assert set(plain.defaults) == set(clipped.defaults) == {"lr", "betas", "eps", "weight_decay"}
    clipped.load_state_dict(a)                                                     # an unclipped optimizer's checkpoint loads
    assert clipped.max_grad_norm == 1.0 and clipped.skip_nonfinite is True


def test_plan_inputs_carry_both_settings():
    m = _model()
    make = lambda **kw: Adam(m.parameters(), capturable="segments", **kw).plan_inputs()
    assert make(max_grad_norm=1.0) != make(max_grad_norm=2.0)
    assert make(max_grad_norm=1.0) != make()
    assert make(skip_nonfinite=True) != make(skip_nonfinite=False)
    assert make(max_grad_norm=1.0, skip_nonfinite=True) != make(max_grad_norm=1.0)
    assert make(max_grad_norm=1.0, skip_nonfinite=True) == make(max_grad_norm=1.0, skip_nonfinite=True)
    assert make() == make()
    opt = Adam(m.parameters(), capturable="segments", max_grad_norm=1.0)
    before = opt.plan_inputs()
    opt.max_grad_norm = 2.0                                                        # what GraphedStep compares before every replay
    assert opt.plan_inputs() != before
