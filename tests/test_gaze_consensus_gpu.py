"""The consensus gaze on the GPU: mvg_gaze_consensus_fwd / _bwd per element against the float64 oracle (tests/gaze_consensus_ref.py:
the definition applied literally, and float64 autograd of it), the skip / degenerate rules by bit equality and exact NaN sets, and
the wiring - forward_multiview(consensus=True), MultiViewConsensusLoss, AngularErrorMeter.update_consensus, InferenceSession.
bind_consensus - by bit equality with the stand-alone launches.

The bar is derived in the oracle module (one fp32 rounding of the result plus double-precision noise): per element
|out - ref| <= 2^-24 |ref| + 1e-12 S, S = 1 for head, views and the resultant, 180 for the spread, the case's max |ref| for dpreds.
Every figure is printed before it is asserted (pytest -s shows them); the measured maxima are in profiles/gaze_consensus_errors.txt."""
import numpy as np
import pytest
import torch

import gaze_consensus_ref as R
import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd import synth

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def _t(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev())        # (a copy: the shared cases are read-only)


def _fwd(preds, rot, w, stats=True):
    from rot_mvgaze_amd import ops
    I, D, B, _ = preds.shape
    V = rot.shape[1]
    mk = lambda *s: torch.full(s, -7.0, dtype=torch.float32, device=dev())
    head, views, st = mk(I, B, 3), mk(I, V, B, 2), (mk(I, B, 2) if stats else None)
    ops.gaze_consensus_fwd(preds, rot, w, I, V, B, head, views, st)
    return head, views, st


def _bwd(dviews, preds, rot, w):
    from rot_mvgaze_amd import ops
    I, D, B, _ = preds.shape
    dpreds = torch.full_like(preds, float("nan"))                                # every row must be written
    ops.gaze_consensus_bwd(dviews, preds, rot, w, I, rot.shape[1], B, dpreds)
    return dpreds


def _bits(a, b):
    """Equal bits (NaN patterns included)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


_CASES = {}


def _case(shape, mode):
    """Inputs and float64 references of one (shape, weights mode), made once for the whole file and never written to."""
    key = (shape, mode)
    if key not in _CASES:
        I, V, B = shape
        preds, rot = R.make_inputs(I, V, B, seed=7)
        w = R.make_weights(mode, V, B, seed=7)
        R.check_conditioning(preds, rot, w)
        dviews = np.random.default_rng(11).normal(size=(I, V, B, 2)).astype(np.float32)
        head, views, stats = R.forward(preds, rot, w)
        c = dict(preds=preds, rot=rot, w=w, dviews=dviews, head=head, views=views, stats=stats,
                 dpreds=R.backward_autograd(dviews, preds, rot, w))
        for a in c.values():
            if a is not None:
                a.setflags(write=False)
        _CASES[key] = c
    return _CASES[key]


def _over(got, ref, scale):
    """max of |got - ref| / bar over the elements (<= 1 passes), and max |got - ref|."""
    err = np.abs(got.astype(np.float64) - ref)
    return float((err / R.bar(ref, scale)).max()), float(err.max())


_IDS = lambda s: "I%d_V%d_B%d" % s if isinstance(s, tuple) else s


# ---------------------------------------------------------------- 1. forward per element
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", R.CASES, ids=_IDS)
def test_forward_per_element(shape, mode):
    c = _case(shape, mode)
    p, r, w = _t(c["preds"]), _t(c["rot"]), _t(c["w"])
    head, views, stats = _fwd(p, r, w, stats=True)
    head0, views0, _ = _fwd(p, r, w, stats=False)
    assert _bits(head, head0) and _bits(views, views0)                           # the same bits with and without stats
    head, views, stats = (a.cpu().numpy() for a in (head, views, stats))
    assert np.isfinite(head).all() and np.isfinite(views).all() and np.isfinite(stats).all() and np.isfinite(c["head"]).all()
    figs = {"head": _over(head, c["head"], 1.0), "views": _over(views, c["views"], 1.0),
            "resultant": _over(stats[..., 0], c["stats"][..., 0], 1.0), "spread": _over(stats[..., 1], c["stats"][..., 1], 180.0)}
    print(f"\nfwd {shape} {mode}: " + "; ".join(f"{k} {v[1]:.3e} ({v[0]:.3f} of the bar)" for k, v in figs.items()))
    for k, v in figs.items():
        assert v[0] <= 1.0, (k, v)


# ---------------------------------------------------------------- 2. skipped means skipped
@pytest.mark.parametrize("shape", [s for s in R.CASES if s[1] > 2], ids=_IDS)
def test_skipped_entries_are_not_read_into_the_sums(shape):
    c = _case(shape, "mask")
    I, V, B = shape
    s, q = R.directed(V)
    masked = [(b, int(np.argmin(c["w"][b]))) for b in range(B) if (c["w"][b] == 0).any()]
    assert masked and len(masked) < B

    def planted(value):
        preds, rot = c["preds"].copy(), c["rot"].copy()
        for b, t in masked:
            for d in range(len(s)):
                if t in (s[d], q[d]):
                    preds[:, d, b] = value                                       # the rows of inactive contributions
            rot[b, t] = value                                                    # a view that takes part in no active contribution
        return _t(preds), _t(rot)
    w, dv = _t(c["w"]), _t(c["dviews"])
    pj, rj = planted(3.0)
    pn, rn = planted(np.nan)
    hj, vj, sj = _fwd(pj, rj, w)
    hn, vn, sn = _fwd(pn, rn, w)
    assert _bits(hj, hn) and _bits(sj, sn) and torch.isfinite(hn).all() and torch.isfinite(vj).all()
    own = torch.zeros(I, V, B, dtype=torch.bool, device=dev())
    for b, t in masked:
        own[:, t, b] = True
    assert torch.isnan(vn[own]).all()                                            # its own rot[b][t] is NaN: a NaN row for that t only
    assert _bits(vj[~own], vn[~own])
    # the untouched inputs give the same head as well (the junk never entered)
    h0, _, _ = _fwd(_t(c["preds"]), _t(c["rot"]), w)
    assert _bits(h0, hn)
    # backward: the same holds for the gradient (a NaN target row is left out, so compare with its dviews zeroed in the junk run)
    dj = dv.clone()
    dj[own] = 0.0
    gj, gn = _bwd(dj, pj, _t(c["rot"]), w), _bwd(dv, pn, rn, w)
    assert torch.isfinite(gn).all() and _bits(gj, gn)


# ---------------------------------------------------------------- 3. degenerate items, planted
def _degenerate_run(preds, rot, w, planted):
    ref_head, ref_views, ref_stats = R.forward(preds, rot, w)
    I, _, B, _ = preds.shape
    want = np.zeros((I, B), dtype=bool)
    for it, b in planted:
        want[it, b] = True
    assert 8 * len(planted) <= I * B
    R.check_conditioning(preds, rot, w, planted)
    assert np.array_equal(np.isnan(ref_head).all(-1), want) and np.array_equal(np.isnan(ref_head).any(-1), want)      # the oracle's set
    p, r, wt = _t(preds), _t(rot), _t(w)
    head, views, stats = (a.cpu().numpy() for a in _fwd(p, r, wt))
    for name, a, axes in (("head", head, (-1,)), ("views", np.moveaxis(views, 1, 2), (-1, -2)), ("stats", stats, (-1,))):
        nan = np.isnan(a)
        assert np.array_equal(nan.all(axes), want) and np.array_equal(nan.any(axes), want), name      # exactly these items, whole rows
    keep = ~want
    assert _over(head[keep], ref_head[keep], 1.0)[0] <= 1.0
    assert _over(np.moveaxis(views, 1, 2)[keep], np.moveaxis(ref_views, 1, 2)[keep], 1.0)[0] <= 1.0
    dv = torch.from_numpy(np.random.default_rng(5).normal(size=views.shape).astype(np.float32)).to(dev())
    g = _bwd(dv, p, r, wt).cpu().numpy()
    assert np.isfinite(g).all()
    assert not np.moveaxis(g, 1, 2)[want].any()                                  # all rows of a degenerate item: exactly 0
    assert (np.abs(np.moveaxis(g, 1, 2)[keep]).max((-1, -2)) > 0).all()
    return g


def test_planted_degenerate_items():
    I, V, B = 3, 4, 40
    preds, rot = R.make_inputs(I, V, B, seed=21)
    w = R.make_weights("confidence", V, B, seed=21)
    preds, rot = preds.copy(), rot.copy()
    w[3, :] = 0.0                                                                # no active contribution
    w[7, 2] = -0.5                                                               # one negative weight
    preds[1, 5, 11, 1] = np.nan                                                  # a NaN in an active preds row (iteration 1 only)
    _degenerate_run(preds, rot, w, [(it, 3) for it in range(I)] + [(it, 7) for it in range(I)] + [(1, 11)])


def test_antipodal_pair_cancels():
    I, V, B = 1, 2, 16
    preds, rot = R.make_inputs(I, V, B, seed=22)
    preds, rot = preds.copy(), rot.copy()
    for b in (5, 12):                                                            # identity rotations, pred_1 = (-p, y + pi)
        rot[b] = np.eye(3, dtype=np.float32)
        preds[0, 1, b] = (-preds[0, 0, b, 0], preds[0, 0, b, 1] + np.float32(np.pi))
    h = R.vec(preds[0, 0, [5, 12]].astype(np.float64)) + R.vec(preds[0, 1, [5, 12]].astype(np.float64))
    print(f"\nantipodal residual |h| / W = {np.linalg.norm(h, axis=-1) / 2}")
    assert (np.linalg.norm(h, axis=-1) / 2 < 1e-6).all()                         # far below the 1e-4 threshold
    _degenerate_run(preds, rot, None, [(0, 5), (0, 12)])


# ---------------------------------------------------------------- 4. backward per element
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", R.CASES, ids=_IDS)
def test_backward_per_element(shape, mode):
    c = _case(shape, mode)
    I, V, B = shape
    g = _bwd(_t(c["dviews"]), _t(c["preds"]), _t(c["rot"]), _t(c["w"])).cpu().numpy()
    assert not np.isnan(g).any() and np.isfinite(g).all()                        # the NaN pre-fill is gone
    scale = float(np.abs(c["dpreds"]).max())
    over, err = _over(g, c["dpreds"], scale)
    print(f"\nbwd {shape} {mode}: max |dpreds - autograd| {err:.3e} at max |ref| {scale:.3e} ({over:.3f} of the bar)")
    assert scale > 1e-3 and over <= 1.0
    if c["w"] is not None:
        s, q = R.directed(V)
        inactive = np.stack([(c["w"][:, s[d]] * c["w"][:, q[d]]) <= 0 for d in range(len(s))])      # [D,B]
        assert inactive.any() == (mode == "mask" and V > 2)
        assert not g[:, inactive].any() and (np.abs(g[:, ~inactive]).max(-1) > 0).all()


# ---------------------------------------------------------------- 5. reproducible, capturable
def test_equal_calls_give_equal_bits_and_a_graph_replays_them():
    c = _case((3, 4, 300), "mask")
    p, r, w, dv = _t(c["preds"]), _t(c["rot"]), _t(c["w"]), _t(c["dviews"])
    a, b = _fwd(p, r, w), _fwd(p, r, w)
    assert all(_bits(x, y) for x, y in zip(a, b))
    assert _bits(_bwd(dv, p, r, w), _bwd(dv, p, r, w))
    from rot_mvgaze_amd import ops
    out = [torch.zeros_like(x) for x in a]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.gaze_consensus_fwd(p, r, w, 3, 4, 300, *out)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.gaze_consensus_fwd(p, r, w, 3, 4, 300, *out)
    for o in out:
        o.fill_(-7.0)
    g.replay()
    torch.cuda.synchronize()
    assert all(_bits(x, y) for x, y in zip(a, out))


# ---------------------------------------------------------------- 6. wiring
def _model(num_iter, compute=torch.float32, train=False):
    from rot_mvgaze_amd.model import MultiViewGaze
    sd = synth.make_state_dict(18, 0, num_iter, perturb_bn=True)
    m = MultiViewGaze(18, num_iter)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    m.to(dev())
    m.train() if train else m.eval()
    m.compute_dtype = compute
    m.ensure_layout()
    return m


def _inputs(B, V, hw=64, seed=1234):
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    inp = synth.make_inputs(B, V, seed, hw)
    img, hp, gt = (torch.from_numpy(inp[k]) for k in ("img", "head_pose", "gt_gaze"))
    imgs = [img[:, v].contiguous().to(dev()) for v in range(V)]
    rot = torch.stack([rotation_matrix_2d(hp[:, v].contiguous().to(dev())) for v in range(V)], dim=1).contiguous()
    return imgs, rot, gt.to(dev())


def test_model_loss_and_meter_wiring():
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd.losses import MultiViewConsensusLoss, _FusedIterLossFn, iteration_weights
    from rot_mvgaze_amd.metrics import AngularErrorMeter
    I, V, B = 2, 3, 2
    m = _model(I)                                                                # eval mode with gradients: two forwards of one batch agree
    imgs, rot, gt = _inputs(B, V)
    wv = torch.tensor([[1.0, 0.5, 2.0], [1.5, 1.0, 0.0]], device=dev())
    plain = m.forward_multiview(imgs, rot)
    assert "consensus" not in plain
    out = m.forward_multiview(imgs, rot, consensus=True, view_weights=wv)
    preds = out["_mvg_preds"]
    assert _bits(preds, plain["_mvg_preds"]) and _bits(out["pred_gaze"], plain["pred_gaze"]) and set(out) == set(plain) | {"consensus"}
    cons = out["consensus"]
    assert set(cons) == {"head", "views", "resultant", "spread", "pred_gaze"}
    head, views, stats = _fwd(preds.detach(), rot, wv)
    assert _bits(cons["views"], views) and _bits(cons["head"], head)
    assert _bits(cons["resultant"], stats[..., 0]) and _bits(cons["spread"], stats[..., 1])
    assert tuple(cons["pred_gaze"].shape) == (B, V, 2) and _bits(cons["pred_gaze"], views[m._output_index].transpose(0, 1))
    assert cons["pred_gaze"].untyped_storage().data_ptr() == cons["views"].untyped_storage().data_ptr()       # a view, no copy
    assert torch.isfinite(views).all()
    from rot_mvgaze_amd.consensus import gaze_consensus
    two = gaze_consensus(preds.detach(), rot, wv)                                # without stats: two outputs, the same bits
    assert len(two) == 2 and _bits(two[0], head) and _bits(two[1], views)
    # the loss: the fused loss launch over the views, one "direction" per view
    crit = MultiViewConsensusLoss(weight=0.01, iter_decay=0.5)
    iw, dw = iteration_weights(I, 0.5, None), [0.01 / V] * V
    gt_dir = gt.to(torch.float32).transpose(0, 1).contiguous()
    loss = crit(out, gt)
    by_hand = _FusedIterLossFn.apply(views, gt_dir, iw, dw)
    assert _bits(loss.detach().reshape(1), by_hand.reshape(1)) and torch.isfinite(loss)
    # its gradient at the pair predictions: the consensus backward of the loss kernel's dpred
    preds.retain_grad()
    loss.backward()
    l2, dpred = torch.empty(1, device=dev()), torch.empty_like(views)
    ops.gaze_angular_loss_multi(views, gt_dir, I, V, B, [iw[it] * dw[t] for it in range(I) for t in range(V)], l2, dpred)
    assert _bits(preds.grad, _bwd(dpred, preds.detach(), rot, wv)) and preds.grad.abs().max() > 0
    s, q = R.directed(V)
    for d in range(len(s)):                                                      # sample 1's view 2 is masked: its rows get exactly 0
        if 2 in (s[d], q[d]):
            assert not preds.grad[:, d, 1].any()
    # the meter
    meter = AngularErrorMeter(num_iter=I, dirs=V, capacity=B, device=dev())
    meter.update_consensus(out, gt)
    rec, eo = torch.zeros(I, V, 5, dtype=torch.float64, device=dev()), torch.empty(I, V, B, dtype=torch.float32, device=dev())
    ops.gaze_error_update(views, gt_dir, I, V, B, rec, eo, B)
    assert torch.equal(meter.record, rec) and _bits(meter.err_out, eo) and (meter.compute()["count"] == B).all()


# ---------------------------------------------------------------- 7. session
@pytest.mark.parametrize("compute", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_session_consensus(compute):
    from rot_mvgaze_amd.session import InferenceSession
    m = _model(3, compute)
    B, V = 2, 3
    imgs, rot, gt = _inputs(B, V)
    kw = dict(compute=torch.bfloat16) if compute == torch.bfloat16 else {}
    with InferenceSession(m, V, B, 64, 64, **kw) as s:
        want = [o.clone() for o in s.run(imgs, rot)]
        launches = s.launches
        assert s.consensus is None
        wv = torch.tensor([[1.0, 0.5, 2.0], [1.5, 0.0, 1.0]], device=dev())
        for weights, stats in ((None, False), (wv, True)):
            s.bind_consensus(weights, stats=stats)
            assert s.launches == launches + 1 and set(s.consensus) == ({"head", "views", "stats"} if stats else {"head", "views"})
            for t in s.consensus.values():
                t.fill_(-7.0)
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                got = s.run(imgs, rot)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            for a, b in zip(got, want):
                assert _bits(a, b)                                               # the four plain outputs are unchanged
            head, views, st = _fwd(got[3], rot, weights, stats=stats)
            assert _bits(s.consensus["head"], head) and _bits(s.consensus["views"], views) and torch.isfinite(views).all()
            assert not stats or _bits(s.consensus["stats"], st)
        held = {k: v.clone() for k, v in s.consensus.items()}
        last = s.consensus
        s.unbind_consensus()
        assert s.launches == launches and s.consensus is None
        for t in last.values():
            t.fill_(-7.0)
        again = s.run(imgs, rot)
        for a, b in zip(again, want):
            assert _bits(a, b)
        assert all((t == -7.0).all() for t in last.values()) and held["views"].ne(-7.0).all()      # the plain forward: nothing written
