"""The gaze error meter's host side (no GPU): the two ABI additions and the record's constants in header, binding and library;
every argument check of mvg_gaze_error_update and mvg_session_set_error_record (they run before any HIP call); the session hook
on a host-built session (one more launch, the plan untouched); AngularErrorMeter refuses host tensors; the meter's label layout
is MultiViewIterationLoss's; and the oracle the GPU file uses is the host metric wherever its clamp is inactive."""
import ctypes as C

import numpy as np
import pytest
import torch

import cabi_header as hdr
import gaze_error_ref as R
import rot_mvgaze_amd  # noqa: F401

FIELDS = ("COUNT", "SUM", "SUMSQ", "MAX", "NONFINITE")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from rot_mvgaze_amd import _lib
    return _lib.lib()


def _err(L):
    return (L.mvg_last_error() or b"").decode()


# ---------------------------------------------------------------- ABI
def test_abi_additions(L):
    from rot_mvgaze_amd import _lib
    assert hdr.functions["mvg_gaze_error_update"] == ("int", [("float*", "preds"), ("float*", "gt"), ("int", "iters"), ("int", "dirs"),
                                                              ("int", "batch"), ("double*", "record"), ("float*", "err_out"),
                                                              ("int64_t", "capacity"), ("void*", "stream")])
    assert hdr.functions["mvg_session_set_error_record"] == ("int", [("mvg_session*", "s"), ("float*", "gt_dev"), ("double*", "record_dev"),
                                                                     ("float*", "err_out"), ("int64_t", "capacity")])
    for name in ("mvg_gaze_error_update", "mvg_session_set_error_record"):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == hdr.arity(name)
        assert hasattr(L, name), f"{name} is not exported"
    for k, f in enumerate(FIELDS):
        assert hdr.constants["MVG_GAZE_ERR_" + f] == getattr(_lib, "GAZE_ERR_" + f) == k
    assert hdr.constants["MVG_GAZE_ERR_FIELDS"] == _lib.GAZE_ERR_FIELDS == len(FIELDS)
    assert hdr.constants["MVG_ABI_VERSION"] == _lib.ABI_VERSION == L.mvg_abi_version() == 13
    assert "mvg_gaze_err" not in " ".join(hdr.structs)           # a plain double array, no new struct


# ---------------------------------------------------------------- argument checks (before any HIP call)
def _update_args(**kw):
    """A well-formed argument list over HOST memory (never dereferenced: each case below is rejected first)."""
    keep = [(C.c_float * 4)(), (C.c_float * 4)(), (C.c_double * 5)(), (C.c_float * 4)()]
    a = dict(preds=C.cast(keep[0], C.c_void_p), gt=C.cast(keep[1], C.c_void_p), iters=1, dirs=1, batch=1,
             record=C.cast(keep[2], C.c_void_p), err_out=None, capacity=0)
    for k, v in kw.items():
        a[k] = C.cast(keep[3], C.c_void_p) if v == "buffer" else v
    return keep, [a[k] for k in ("preds", "gt", "iters", "dirs", "batch", "record", "err_out", "capacity")] + [None]


@pytest.mark.parametrize("bad, word", [(dict(preds=None), "null"), (dict(gt=None), "null"), (dict(record=None), "null"),
                                       (dict(iters=0), "iters"), (dict(dirs=0), "dirs"), (dict(batch=0), "batch"),
                                       (dict(iters=-3), "iters"), (dict(capacity=-1), "capacity"),
                                       (dict(err_out="buffer", capacity=0), "capacity")])
def test_update_rejects_bad_arguments(L, bad, word):
    keep, a = _update_args(**bad)
    assert L.mvg_session_set_error_record(None, None, None, None, 0) != 0       # (another call's message is in place first)
    rc = L.mvg_gaze_error_update(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8])
    assert rc != 0
    assert _err(L).startswith("gaze_error_update:") and word in _err(L), _err(L)


# ---------------------------------------------------------------- the fused loss launch's 512-cell limit
def _loss_multi(L, iters, dirs):
    """mvg_gaze_angular_loss_multi at batch 1.  The weights travel by value in a float[512] kernel argument, so iters * dirs is
    checked before any HIP call.  On a machine with a GPU the tensors are device memory (an accepted call does launch);
    without one the launch cannot happen and the host buffers are never read."""
    n = iters * dirs
    w = (C.c_float * n)()
    if torch.cuda.is_available():
        keep = [torch.zeros(n, 1, 2, device="cuda") + 0.1, torch.zeros(dirs, 1, 2, device="cuda"), torch.zeros(1, device="cuda")]
        ptr = [C.c_void_p(t.data_ptr()) for t in keep]
    else:
        keep = [(C.c_float * (2 * n))(), (C.c_float * (2 * dirs))(), (C.c_float * 1)()]
        ptr = [C.cast(b, C.c_void_p) for b in keep]
    rc = L.mvg_gaze_angular_loss_multi(ptr[0], ptr[1], iters, dirs, 1, w, ptr[2], None, None)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return rc, _err(L)


@pytest.mark.parametrize("iters, dirs", [(9, 57), (1, 513), (513, 1), (27, 19)])
def test_loss_launch_rejects_513_cells(L, iters, dirs):
    assert iters * dirs == 513
    assert L.mvg_session_set_error_record(None, None, None, None, 0) != 0       # (another call's message is in place first)
    rc, msg = _loss_multi(L, iters, dirs)
    assert rc != 0
    assert msg.startswith("gaze_angular_loss_multi: bad arguments") and "iters * dirs <= 512" in msg, msg


@pytest.mark.parametrize("iters, dirs", [(8, 64), (512, 1), (1, 512)])
def test_loss_launch_takes_512_cells(L, iters, dirs):
    """Exactly 512 cells pass the argument check: with a GPU the call succeeds, without one the only complaint is the missing
    device (the runtime's, from the launch that follows the checks)."""
    assert iters * dirs == 512
    assert L.mvg_session_set_error_record(None, None, None, None, 0) != 0
    rc, msg = _loss_multi(L, iters, dirs)
    if torch.cuda.is_available():
        assert rc == 0, msg
    else:
        assert "bad arguments" not in msg and "512" not in msg, msg
        assert rc != 0 and msg.startswith("gaze_angular_loss_multi:") and "device" in msg, msg


# ---------------------------------------------------------------- the session hook on a host-built session
def _cfg(**kw):
    from rot_mvgaze_amd._lib import SessionCfg
    d = dict(depth=18, num_iter=3, views=2, batch=2, height=64, width=64, share_weights=0, ignore_rotmat=0, split=1, raw_u8=0,
             in_h=0, in_w=0, input_bgr=0)
    d.update(kw)
    return SessionCfg(**d)


def test_set_error_record_rejects_a_null_session(L):
    assert L.mvg_session_set_error_record(None, None, None, None, 0) != 0
    assert "null session" in _err(L)


@pytest.mark.parametrize("compute", [0, 1])
def test_session_hook_adds_one_launch_and_leaves_the_plan(L, compute):
    h = C.c_void_p()
    assert L.mvg_session_create_ex(C.byref(_cfg()), compute, C.byref(h)) == 0, _err(L)
    try:
        def plan():
            return [L.mvg_session_step_name(h, i) for i in range(L.mvg_session_num_steps(h))]
        launches, steps = L.mvg_session_launches(h), plan()
        assert launches == len(steps) > 10
        gt, rec, eo = (C.c_float * 8)(), (C.c_double * 30)(), (C.c_float * 42)()      # stored only (host memory is never read here)
        P = lambda b: C.cast(b, C.c_void_p)
        assert L.mvg_session_set_error_record(h, P(gt), P(rec), None, 0) == 0, _err(L)
        assert L.mvg_session_launches(h) == launches + 1 and plan() == steps
        assert L.mvg_session_set_error_record(h, P(gt), P(rec), P(eo), 7) == 0, _err(L)
        assert L.mvg_session_launches(h) == launches + 1 and plan() == steps
        # rejected settings leave the hook as it was
        assert L.mvg_session_set_error_record(h, None, P(rec), None, 0) != 0 and "gt_dev" in _err(L)
        assert L.mvg_session_set_error_record(h, P(gt), P(rec), P(eo), 0) != 0 and "capacity" in _err(L)
        assert L.mvg_session_set_error_record(h, P(gt), P(rec), None, -1) != 0 and "capacity" in _err(L)
        assert L.mvg_session_launches(h) == launches + 1
        assert L.mvg_session_set_error_record(h, None, None, None, 0) == 0, _err(L)
        assert L.mvg_session_launches(h) == launches and plan() == steps
    finally:
        L.mvg_session_destroy(h)


# ---------------------------------------------------------------- Python
def test_meter_refuses_host_tensors():
    from rot_mvgaze_amd.metrics import AngularErrorMeter
    assert rot_mvgaze_amd.AngularErrorMeter is AngularErrorMeter and rot_mvgaze_amd.metrics.AngularErrorMeter is AngularErrorMeter
    m = AngularErrorMeter()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.update(torch.zeros(4, 2), torch.zeros(4, 2))
    m = AngularErrorMeter(num_iter=3, dirs=2)
    data = {"_mvg_preds": torch.zeros(3, 2, 4, 2), "gt_gaze": torch.zeros(4, 2), "gt_gaze_1": torch.zeros(4, 2)}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.update(data)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        AngularErrorMeter(device="cpu")
    with pytest.raises(ValueError):
        m.update(torch.zeros(4, 3), torch.zeros(4, 3))          # 3-vectors are out of scope
    c = AngularErrorMeter(num_iter=3, dirs=2).compute()         # an empty meter reads as empty, with no device
    assert np.isnan(c["error_gaze"]) and c["count"].shape == (3, 2) and not c["count"].any()


@pytest.mark.parametrize("V", [2, 3])
def test_gt_dir_is_the_loss_modules_layout(V, monkeypatch):
    """build_gt_dir against what MultiViewIterationLoss hands its fused loss (captured in front of the kernel call)."""
    from rot_mvgaze_amd import losses
    from rot_mvgaze_amd.metrics import build_gt_dir
    seen = {}

    class Capture:
        @staticmethod
        def apply(preds, gt_dir, iw, dw):
            seen["gt_dir"] = gt_dir
            return preds.sum()

    monkeypatch.setattr(losses, "_FusedIterLossFn", Capture)
    B, D = 5, V * (V - 1)
    gt = torch.from_numpy(np.random.default_rng(V).uniform(-1, 1, size=(B, V, 2)).astype(np.float32))
    losses.MultiViewIterationLoss()({"_mvg_preds": torch.zeros(3, D, B, 2), "views": V}, gt)
    got = build_gt_dir(gt, V)
    assert got.shape == (D, B, 2) and got.dtype == torch.float32 and torch.equal(got, seen["gt_dir"])
    vi = [i for a in range(V) for b in range(a + 1, V) for i in (a, b)]          # direction d predicts for view vi[d]
    for d in range(D):
        assert torch.equal(got[d], gt[:, vi[d]])
    with pytest.raises(ValueError):
        build_gt_dir(gt, V + 1)


def test_oracle_is_the_host_metric():
    """gaze_error_ref.oracle == geometry.angular_error (float64) bit for bit wherever the host metric is finite, and 0 where it
    is NaN (pred == gt: the similarity rounded past 1)."""
    from rot_mvgaze_amd.geometry import angular_error
    preds, gt = R.make_inputs(3, 2, 300, 11)
    p, g = preds.reshape(-1, 2).astype(np.float64), np.tile(gt.reshape(-1, 2), (3, 1)).astype(np.float64)
    assert np.array_equal(R.oracle(p, g), angular_error(p, g))
    with np.errstate(invalid="ignore"):
        same = angular_error(g, g)
    assert np.isnan(same).any()                                  # the reason for the clamp
    ours = R.oracle(g, g)
    assert np.array_equal(ours[~np.isnan(same)], same[~np.isnan(same)]) and not ours[np.isnan(same)].any()
    assert (R.oracle(p, g) < R.FLOOR_DEG).mean() <= R.MAX_EXCLUDED
