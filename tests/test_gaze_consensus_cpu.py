"""The consensus gaze's host side (no GPU): the three ABI additions in header, binding and library; every argument check of
mvg_gaze_consensus_fwd / _bwd (they run before any HIP call); mvg_session_set_consensus on a host-built session (one more launch,
the plan untouched); the Python entry points refuse host tensors; and the oracle the GPU file uses checks itself: its analytic
backward against float64 autograd, the V = 2 closed form, consistent predictions, and invariance under a common rotation."""
import ctypes as C

import numpy as np
import pytest
import torch

import cabi_header as hdr
import gaze_consensus_ref as R
import rot_mvgaze_amd  # noqa: F401


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
    assert hdr.functions["mvg_gaze_consensus_fwd"] == ("int", [("float*", "preds"), ("float*", "rot"), ("float*", "weights"), ("int", "iters"),
                                                               ("int", "views"), ("int", "batch"), ("float*", "head"),
                                                               ("float*", "views_out"), ("float*", "stats"), ("void*", "stream")])
    assert hdr.functions["mvg_gaze_consensus_bwd"] == ("int", [("float*", "dviews"), ("float*", "preds"), ("float*", "rot"),
                                                               ("float*", "weights"), ("int", "iters"), ("int", "views"), ("int", "batch"),
                                                               ("float*", "dpreds"), ("void*", "stream")])
    assert hdr.functions["mvg_session_set_consensus"] == ("int", [("mvg_session*", "s"), ("float*", "weights_dev"), ("float*", "head"),
                                                                  ("float*", "views_out"), ("float*", "stats")])
    P, I = C.c_void_p, C.c_int
    want = {"mvg_gaze_consensus_fwd": [P, P, P, I, I, I, P, P, P, P], "mvg_gaze_consensus_bwd": [P, P, P, P, I, I, I, P, P],
            "mvg_session_set_consensus": [P, P, P, P, P]}
    for name, args in want.items():
        assert _lib.SIGNATURES[name] == (I, args) and len(args) == hdr.arity(name)
        assert hasattr(L, name), f"{name} is not exported"
    assert hdr.constants["MVG_ABI_VERSION"] == _lib.ABI_VERSION == L.mvg_abi_version() == 13


# ---------------------------------------------------------------- argument checks (before any HIP call)
_FWD = ("preds", "rot", "weights", "iters", "views", "batch", "head", "views_out", "stats")
_BWD = ("dviews", "preds", "rot", "weights", "iters", "views", "batch", "dpreds")


def _args(names, **kw):
    """A well-formed argument list over HOST memory (never dereferenced: each case below is rejected first)."""
    keep = {n: (C.c_double * 16)() for n in names if n not in ("iters", "views", "batch")}      # (doubles: 8-byte aligned)
    a = {n: C.cast(b, C.c_void_p) for n, b in keep.items()}
    a.update(iters=1, views=2, batch=1)
    a.update(kw)
    return keep, [a[n] for n in names] + [None]


_BAD_SIZES = [(dict(views=1), "views"), (dict(views=9), "views"), (dict(views=-2), "views"), (dict(iters=0), "iters"),
              (dict(iters=-3), "iters"), (dict(batch=0), "batch"), (dict(iters=2 ** 16, batch=2 ** 15), "one grid"),
              (dict(iters=2 ** 31 - 1, batch=2 ** 31 - 1), "one grid")]


@pytest.mark.parametrize("bad, word", [(dict(preds=None), "preds"), (dict(rot=None), "rot"), (dict(head=None), "head"),
                                       (dict(views_out=None), "views_out")] + _BAD_SIZES)
def test_fwd_rejects_bad_arguments(L, bad, word):
    keep, a = _args(_FWD, **bad)
    assert L.mvg_session_set_consensus(None, None, None, None, None) != 0       # (another call's message is in place first)
    assert L.mvg_gaze_consensus_fwd(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9]) != 0
    assert _err(L).startswith("gaze_consensus_fwd:") and word in _err(L), _err(L)


@pytest.mark.parametrize("bad, word", [(dict(dviews=None), "dviews"), (dict(preds=None), "preds"), (dict(rot=None), "rot"),
                                       (dict(dpreds=None), "dpreds")] + _BAD_SIZES)
def test_bwd_rejects_bad_arguments(L, bad, word):
    keep, a = _args(_BWD, **bad)
    assert L.mvg_session_set_consensus(None, None, None, None, None) != 0
    assert L.mvg_gaze_consensus_bwd(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]) != 0
    assert _err(L).startswith("gaze_consensus_bwd:") and word in _err(L), _err(L)


def test_optional_arguments_pass_the_checks(L):
    """weights = NULL and stats = NULL are legal: without a GPU the only complaint is the runtime's, from the launch that follows
    the checks; with one the call runs (device buffers)."""
    if torch.cuda.is_available():
        t = [torch.zeros(32, device="cuda") for _ in range(4)]                   # preds 4, rot 18, head 3, views_out 4 floats are read / written
        t[1][:18] = torch.eye(3, device="cuda").reshape(-1).repeat(2)
        rc = L.mvg_gaze_consensus_fwd(C.c_void_p(t[0].data_ptr()), C.c_void_p(t[1].data_ptr()), None, 1, 2, 1, C.c_void_p(t[2].data_ptr()),
                                      C.c_void_p(t[3].data_ptr()), None, None)
        torch.cuda.synchronize()
        assert rc == 0, _err(L)
    else:
        keep, a = _args(_FWD, weights=None, stats=None)
        assert L.mvg_gaze_consensus_fwd(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9]) != 0
        msg = _err(L)
        assert msg.startswith("gaze_consensus_fwd:") and "null" not in msg and "must be" not in msg and "device" in msg, msg


# ---------------------------------------------------------------- the session hook on a host-built session
def _cfg(**kw):
    from rot_mvgaze_amd._lib import SessionCfg
    d = dict(depth=18, num_iter=3, views=3, batch=2, height=64, width=64, share_weights=0, ignore_rotmat=0, split=1, raw_u8=0,
             in_h=0, in_w=0, input_bgr=0)
    d.update(kw)
    return SessionCfg(**d)


def test_set_consensus_rejects_a_null_session(L):
    assert L.mvg_session_set_consensus(None, None, None, None, None) != 0
    assert "null session" in _err(L) and _err(L).startswith("session_set_consensus:")


@pytest.mark.parametrize("compute", [0, 1])
def test_session_hook_adds_one_launch_and_leaves_the_plan(L, compute):
    h = C.c_void_p()
    assert L.mvg_session_create_ex(C.byref(_cfg()), compute, C.byref(h)) == 0, _err(L)
    try:
        def plan():
            return [L.mvg_session_step_name(h, i) for i in range(L.mvg_session_num_steps(h))]
        launches, steps = L.mvg_session_launches(h), plan()
        assert launches == len(steps) > 10
        bufs = [(C.c_float * 64)() for _ in range(6)]                       # stored only (host memory is never read here)
        w, head, views, stats, gt, rec = (C.cast(b, C.c_void_p) for b in bufs)
        assert L.mvg_session_set_consensus(h, None, head, views, None) == 0, _err(L)
        assert L.mvg_session_launches(h) == launches + 1 and plan() == steps
        assert L.mvg_session_set_consensus(h, w, head, views, stats) == 0, _err(L)
        assert L.mvg_session_launches(h) == launches + 1 and plan() == steps
        # next to the error record: one launch each
        assert L.mvg_session_set_error_record(h, gt, rec, None, 0) == 0, _err(L)
        assert L.mvg_session_launches(h) == launches + 2 and plan() == steps
        assert L.mvg_session_set_error_record(h, None, None, None, 0) == 0, _err(L)
        # a rejected setting leaves the hook as it was
        assert L.mvg_session_set_consensus(h, None, None, views, None) != 0 and "head" in _err(L)
        assert L.mvg_session_launches(h) == launches + 1
        assert L.mvg_session_set_consensus(h, None, None, None, None) == 0, _err(L)
        assert L.mvg_session_launches(h) == launches and plan() == steps and L.mvg_session_num_steps(h) == len(steps)
    finally:
        L.mvg_session_destroy(h)


# ---------------------------------------------------------------- Python
def test_python_entry_points_refuse_host_tensors():
    from rot_mvgaze_amd.consensus import gaze_consensus
    from rot_mvgaze_amd.metrics import AngularErrorMeter
    from rot_mvgaze_amd.model import MultiViewGaze
    assert rot_mvgaze_amd.gaze_consensus is gaze_consensus and rot_mvgaze_amd.consensus.gaze_consensus is gaze_consensus
    assert rot_mvgaze_amd.MultiViewConsensusLoss is rot_mvgaze_amd.losses.MultiViewConsensusLoss
    preds, rot = (torch.from_numpy(a) for a in R.make_inputs(3, 3, 4, 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gaze_consensus(preds, rot)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gaze_consensus(preds, rot, torch.ones(4, 3), stats=True)
    m = AngularErrorMeter(num_iter=3, dirs=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.update_consensus({"consensus": {"views": torch.zeros(3, 3, 4, 2)}}, torch.zeros(4, 3, 2))
    with pytest.raises(ValueError):
        m.update_consensus({"_mvg_preds": preds}, torch.zeros(4, 3, 2))    # not a consensus=True output
    model = MultiViewGaze(18, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.forward_multiview([torch.zeros(1, 3, 64, 64)] * 3, torch.eye(3).repeat(1, 3, 1, 1), consensus=True)


# ---------------------------------------------------------------- the oracle checks itself
@pytest.mark.parametrize("shape, mode", [((3, 2, 5), "confidence"), ((2, 3, 7), "mask"), ((3, 4, 9), "mask"), ((1, 8, 3), "none")])
def test_analytic_backward_is_autograd(shape, mode):
    I, V, B = shape
    preds, rot = R.make_inputs(I, V, B, seed=5)
    w = R.make_weights(mode, V, B, seed=5)
    preds, rot = preds.copy(), rot.copy()
    if mode == "mask":
        w[1, :] = 0.0                                                       # a degenerate item: no active contribution
        b = 0                                                               # sample 0 is masked: NaN where the definition skips
        t = int(np.argmin(w[b]))
        s, q = R.directed(V)
        for d in range(len(s)):
            if t in (s[d], q[d]):
                preds[:, d, b] = np.nan
        rot[b, t] = np.nan
    dviews = np.random.default_rng(9).normal(size=(I, V, B, 2)).astype(np.float32)
    a, g = R.backward_analytic(dviews, preds, rot, w), R.backward_autograd(dviews, preds, rot, w)
    assert np.isfinite(a).all() and np.isfinite(g).all() and np.abs(a).max() > 1e-3
    assert np.abs(a - g).max() <= 1e-12, np.abs(a - g).max()
    if mode == "mask":
        assert not a[:, :, 1].any() and not g[:, :, 1].any()
        head, views, stats = R.forward(preds, rot, w)
        assert np.isnan(head[:, 1]).all() and np.isnan(views[:, :, 1]).all() and np.isnan(stats[:, 1]).all()
        assert np.isnan(views[:, t, 0]).all() and np.isfinite(np.delete(views[:, :, 0], t, axis=1)).all() and np.isfinite(head[:, 0]).all()


def test_two_view_closed_form():
    """V = 2: the consensus in view 0 is the normalised mean of pred_0 and rot_0 rot_1^T pred_1."""
    preds, _ = R.make_inputs(3, 2, 6, seed=2)
    r = R.rotation(np.random.default_rng(2).uniform(-0.5, 0.5, size=(6, 2, 2)))     # float64: orthogonal to 1e-16, not to 6e-8
    head, views, _ = R.forward(preds, r)
    p = preds.astype(np.float64)
    rel = np.einsum("bkm,bnm->bkn", r[:, 0], r[:, 1])                       # rot_0 rot_1^T
    mean = R.vec(p[:, 0]) + np.einsum("bkn,ibn->ibk", rel, R.vec(p[:, 1]))
    mean /= np.linalg.norm(mean, axis=-1, keepdims=True)
    assert np.abs(R.to_pitchyaw(mean) - views[:, 0]).max() <= 1e-12


def test_consistent_predictions_return_themselves():
    for V in (2, 4):
        preds, rot = R.make_inputs(2, V, 5, seed=3, noise=0.0, dtype=np.float64)
        head, views, stats = R.forward(preds, rot, R.make_weights("mask", V, 5, seed=3))
        s, _ = R.directed(V)
        for d, t in enumerate(s):
            assert np.abs(views[:, t] - preds[:, d]).max() <= 1e-12
        # (acos next to 1: a similarity of 1 - k 2^-53 reads as sqrt(2 k) 1.05e-8 rad = sqrt(k) 8.5e-7 degrees)
        assert np.abs(stats[..., 0] - 1.0).max() <= 1e-12 and stats[..., 1].max() <= 1e-5


def test_a_common_rotation_leaves_the_views_unchanged():
    """Composing every rot[b][t] with one fixed rotation of the HEAD frame (rot[b][t] @ Q, under which rel = rot_i rot_j^T - all the
    model sees - is unchanged) turns ``head`` by Q^T and leaves ``views`` and ``stats`` as they were.  (The product in the other
    order, Q @ rot[b][t], turns every camera frame while the predictions stay: that is a different input, and the definition is
    not invariant under it - h becomes sum w rot_s^T Q^T v_d - as the last assertion records.)"""
    preds, rot = R.make_inputs(2, 3, 5, seed=4)
    w = R.make_weights("confidence", 3, 5, seed=4)
    Q = R.rotation(np.array([0.3, -0.7]))
    r64 = rot.astype(np.float64)                                            # (Q's products are not rounded to fp32)
    head, views, stats = R.forward(preds, r64, w)
    head2, views2, stats2 = R.forward(preds, r64 @ Q, w)
    assert np.abs(views - views2).max() <= 1e-12 and np.abs(stats[..., 0] - stats2[..., 0]).max() <= 1e-12
    assert np.abs(stats[..., 1] - stats2[..., 1]).max() <= 1e-9 and np.abs(head2 - head @ Q).max() <= 1e-12
    _, views3, _ = R.forward(preds, Q @ r64, w)
    assert np.abs(views - views3).max() > 1e-3
