"""The gaze error meter on the GPU: mvg_gaze_error_update, metrics.AngularErrorMeter and the session hook against the float64 host
metric (tests/gaze_error_ref.py: geometry.angular_error's formula with the meter's clamp).

The bars.  Double path, per element: |device - oracle| <= 1e-8 deg on rows whose oracle error is >= 0.01 deg (two float64
evaluation orders of the reference's formula differ by at most 9e-11 deg on such rows; the bar leaves ~100x for the device math
library); rows below 0.01 deg are outside that bar and may be at most 1 % of a case's rows.  The fp32 per-sample store: one fp32
rounding of the oracle's value (half a unit in its last place) on top of the double bar.  Accumulated SUM / SUMSQ: 1e-12 relative.
Every figure is printed before it is asserted (pytest -s shows them).  Measured on an MI355X (profiles/gaze_error_meter_errors.txt):
double path at most 5.9e-11 deg per row, SUM 2.1e-13 and SUMSQ 8.9e-16 relative, antipodal rows 7.5e-6 deg from the oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

import gaze_error_ref as R
import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd import synth

pytestmark = pytest.mark.gpu
COUNT, SUM, SUMSQ, MAX, NONFINITE = range(5)


def dev():
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.array(a)).to(dev())               # (a copy: the shared cases are read-only)


_CASES = {}


def _case(shape):
    """(preds, gt_dir, oracle [I,D,B]) of one shape, made once for the whole file and never written to."""
    if shape not in _CASES:
        preds, gt = R.make_inputs(*shape, seed=7)
        want = R.oracle_cells(preds, gt)
        for a in (preds, gt, want):
            a.setflags(write=False)
        _CASES[shape] = (preds, gt, want)
    return _CASES[shape]


def _update(preds, gt, record, err_out=None, capacity=0):
    from rot_mvgaze_amd import ops
    I, D, B, _ = preds.shape
    ops.gaze_error_update(preds, gt, I, D, B, record, err_out, capacity)


def _record(I, D):
    return torch.zeros(I, D, 5, dtype=torch.float64, device=dev())


def _fp32_bar(want):
    return 0.5 * np.spacing(want.astype(np.float32)).astype(np.float64) + R.PER_ELEMENT_BAR_DEG


# ---------------------------------------------------------------- 1. per element
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "I%d_D%d_B%d" % s)
def test_per_element(shape):
    I, D, B = shape
    preds, gt, want = _case(shape)
    p, g = _t(preds), _t(gt)
    # the double path: one single-row update per row, each into a record of its own; SUM of a one-row cell IS the row's error
    recs = torch.zeros(B, I, D, 5, dtype=torch.float64, device=dev())
    for b in range(B):
        _update(p[:, :, b:b + 1].contiguous(), g[:, b:b + 1].contiguous(), recs[b])
    # the fp32 store of one whole-batch update
    rec, eo = _record(I, D), torch.full((I, D, B), -1.0, dtype=torch.float32, device=dev())
    _update(p, g, rec, eo, B)
    recs, rec, eo = recs.cpu().numpy(), rec.cpu().numpy(), eo.cpu().numpy()
    got = np.moveaxis(recs[..., SUM], 0, -1)                     # [I,D,B]
    assert (recs[..., COUNT] == 1).all() and (recs[..., NONFINITE] == 0).all()
    assert np.array_equal(np.moveaxis(recs[..., MAX], 0, -1), got) and np.array_equal(np.moveaxis(recs[..., SUMSQ], 0, -1), got * got)
    held = want >= R.FLOOR_DEG
    dev_max = np.abs(got - want)[held].max()
    f32_max = (np.abs(eo.astype(np.float64) - want) - _fp32_bar(want))[held].max()
    print(f"\n{shape}: max |device - oracle| = {dev_max:.3e} deg on {held.sum()} rows >= {R.FLOOR_DEG} deg "
          f"({(~held).mean():.2%} below, max deviation there {np.abs(got - want)[~held].max() if (~held).any() else 0.0:.3e}); "
          f"fp32 store over its bar by {f32_max:.3e}")
    assert (~held).mean() <= R.MAX_EXCLUDED
    assert np.isfinite(got).all() and (got >= 0).all()
    assert dev_max <= R.PER_ELEMENT_BAR_DEG
    assert f32_max <= 0
    # the whole-batch update saw the same rows: its store is the fp32 rounding of the single-row values, bit for bit
    assert np.array_equal(eo, got.astype(np.float32))
    assert (rec[..., COUNT] == B).all() and np.array_equal(rec[..., MAX], got.max(-1))


# ---------------------------------------------------------------- 2. edge rows
def test_edge_rows():
    rng = np.random.default_rng(3)
    gt = rng.uniform(-1.2, 1.2, size=(1, 300, 2)).astype(np.float32)
    # pred == gt bit for bit: exactly 0, never NaN (the reference's similarity rounds past 1 on some of these rows)
    rec, eo = _record(1, 1), torch.full((1, 1, 300), -1.0, dtype=torch.float32, device=dev())
    _update(_t(gt[None]), _t(gt), rec, eo, 300)
    r = rec.cpu().numpy()[0, 0]
    assert r.tolist() == [300.0, 0.0, 0.0, 0.0, 0.0] and not eo.cpu().numpy().any()
    # antipodal pairs: pitch negated, yaw + fp32 pi
    anti = np.stack([-gt[0, :, 0], gt[0, :, 1] + np.float32(np.pi)], axis=1).astype(np.float32)
    want = R.oracle(anti, gt[0])
    rec, eo = _record(1, 1), torch.empty(1, 1, 300, dtype=torch.float32, device=dev())
    _update(_t(anti[None, None]), _t(gt), rec, eo, 300)
    got = eo.cpu().numpy()[0, 0].astype(np.float64)
    print(f"\nantipodal: oracle {want.min():.6f} .. {want.max():.6f} deg, max |device - oracle| {np.abs(got - want).max():.3e}")
    assert want.min() > 179.99 and np.abs(got - want).max() <= 1e-4
    assert abs(rec.cpu().numpy()[0, 0, MAX] - want.max()) <= 1e-4
    # a NaN row and an Inf row among finite ones
    preds, g2, _ = _case((3, 2, 5))
    preds, g2 = preds.copy(), g2.copy()
    preds[:, :, 1, 0] = np.nan
    g2[:, 3, 1] = np.inf
    want = R.oracle_cells(np.nan_to_num(preds, nan=0.0), np.nan_to_num(g2, posinf=0.0))
    want[:, :, [1, 3]] = np.nan
    rec, eo = _record(3, 2), torch.zeros(3, 2, 5, dtype=torch.float32, device=dev())
    _update(_t(preds), _t(g2), rec, eo, 5)
    r, e = rec.cpu().numpy(), eo.cpu().numpy()
    assert (r[..., NONFINITE] == 2).all() and (r[..., COUNT] == 3).all()
    assert np.isnan(e[:, :, [1, 3]]).all() and np.isfinite(e[:, :, [0, 2, 4]]).all()
    ref = R.record_of(want)
    # (three finite rows per cell, each within the per-element bar)
    assert np.abs(r[..., SUM] - ref[..., SUM]).max() <= 3 * R.PER_ELEMENT_BAR_DEG and np.abs(r[..., MAX] - ref[..., MAX]).max() <= R.PER_ELEMENT_BAR_DEG
    assert np.isfinite(r).all()


# ---------------------------------------------------------------- 3. accumulation, 5. reproducibility
def _three_updates(meter):
    preds, gt, want = _case((3, 2, 300))
    for lo, hi in ((0, 5), (5, 262), (262, 300)):                # one small, one that wraps the 256-thread stride, one ragged
        meter.update({"_mvg_preds": _t(preds[:, :, lo:hi]), "gt_gaze": _t(gt[0, lo:hi]), "gt_gaze_1": _t(gt[1, lo:hi])})
    return want


def test_accumulation_and_reset():
    from rot_mvgaze_amd.metrics import AngularErrorMeter
    m = AngularErrorMeter(num_iter=3, dirs=2, capacity=300, device=dev())
    want = _three_updates(m)
    r, ref = m.record.cpu().numpy(), R.record_of(want)
    rel = lambda k: np.abs(r[..., k] / ref[..., k] - 1.0).max()
    per_row = m.errors()
    print(f"\naccumulated: SUM rel {rel(SUM):.3e}, SUMSQ rel {rel(SUMSQ):.3e}, |MAX - oracle| {np.abs(r[..., MAX] - ref[..., MAX]).max():.3e}")
    assert np.array_equal(r[..., COUNT], ref[..., COUNT]) and (r[..., COUNT] == 300).all() and not r[..., NONFINITE].any()
    assert rel(SUM) <= 1e-12 and rel(SUMSQ) <= 1e-12
    # MAX is the maximum of the per-element values: the store holds their fp32 roundings (monotone), the oracle bounds the rest
    assert per_row.shape == (3, 2, 300) and np.array_equal(r[..., MAX].astype(np.float32), per_row.max(-1))
    assert np.abs(r[..., MAX] - ref[..., MAX]).max() <= R.PER_ELEMENT_BAR_DEG
    c = m.compute()
    assert abs(c["error_gaze"] - want[-1, 0].mean()) <= R.PER_ELEMENT_BAR_DEG and not m.overflowed()
    assert np.abs(c["mean"] - want.mean(-1)).max() <= R.PER_ELEMENT_BAR_DEG and np.abs(c["std"] - want.std(-1)).max() <= 1e-7
    assert np.array_equal(c["count"], np.full((3, 2), 300)) and not c["nonfinite"].any()
    m.reset()
    assert not m.record.cpu().numpy().any() and m.errors().shape == (3, 2, 0)


def test_same_updates_give_the_same_bits():
    from rot_mvgaze_amd.metrics import AngularErrorMeter
    a, b = (AngularErrorMeter(num_iter=3, dirs=2, capacity=300, device=dev()) for _ in range(2))
    _three_updates(a)
    _three_updates(b)
    assert torch.equal(a.record, b.record) and torch.equal(a.err_out, b.err_out) and a.record[..., COUNT].eq(300).all()


# ---------------------------------------------------------------- 4. store bounds
def test_store_stops_at_capacity():
    preds, gt, want = _case((3, 2, 5))
    cap, guard = 7, 3
    buf = torch.full((6, cap + guard), -7.0, dtype=torch.float32, device=dev())      # [cell][capacity | guard] in ONE allocation
    rec = _record(3, 2)
    from rot_mvgaze_amd import _lib, ops
    p, g = _t(preds), _t(gt)
    for _ in range(2):        # one call per cell (iters = dirs = 1), so that each row of the store can sit in front of its own guard
        for cell in range(6):
            i, d = divmod(cell, 2)
            _lib.check(_lib.lib().mvg_gaze_error_update(C.c_void_p(p[i, d].data_ptr()), C.c_void_p(g[d].data_ptr()),
                                                        1, 1, 5, C.c_void_p(rec[i, d].data_ptr()), C.c_void_p(buf[cell].data_ptr()), cap,
                                                        C.c_void_p(ops._s())), "gaze_error_update")
    b, r = buf.cpu().numpy(), rec.cpu().numpy()
    w = want.reshape(6, 5)
    assert (np.abs(b[:, :5].astype(np.float64) - w) <= _fp32_bar(w)).all()            # slots 0..4 = the first update, in order
    assert np.array_equal(b[:, 5:7], b[:, :2])                                        # slots 5, 6 = rows 0, 1 of the second update
    assert (b[:, cap:] == -7.0).all()                                                 # rows 2..4 were not written anywhere
    assert (r[..., COUNT] == 10).all() and not r[..., NONFINITE].any()
    # and through the meter, with the rows packed [cells][capacity] (a row's overflow would land in the next cell's slots)
    from rot_mvgaze_amd.metrics import AngularErrorMeter
    m = AngularErrorMeter(num_iter=3, dirs=2, capacity=cap, device=dev())
    m.err_out.fill_(-7.0)
    data = {"_mvg_preds": p, "gt_gaze": g[0], "gt_gaze_1": g[1]}
    m.update(data)
    first = m.err_out.cpu().numpy().copy()
    assert (first[..., 5:] == -7.0).all() and not m.overflowed()
    m.update(data)
    e = m.errors()
    assert e.shape == (3, 2, cap) and np.array_equal(e[..., :5], first[..., :5]) and np.array_equal(e[..., 5:], first[..., :2])
    assert m.overflowed() and (m.compute()["count"] == 10).all()


# ---------------------------------------------------------------- 6. no sync, capturable
def test_update_does_not_synchronise_and_replays_from_a_graph():
    from rot_mvgaze_amd.metrics import AngularErrorMeter
    preds, gt, want = _case((2, 6, 64))
    V, B = 3, 64
    vi = [0, 1, 0, 2, 1, 2]
    labels = np.zeros((B, V, 2), dtype=np.float32)               # gt [B,V,2] whose build_gt_dir is this case's gt_dir
    for d, v in enumerate(vi):
        labels[:, v] = gt[d]                                     # (a view keeps the last of its directions' rows)
    gt_dir = np.stack([labels[:, v] for v in vi])
    want = R.oracle_cells(preds, gt_dir)
    batches = [(np.roll(preds, k, axis=2), np.roll(labels, k, axis=0)) for k in range(3)]
    eager = AngularErrorMeter(num_iter=2, dirs=6, capacity=3 * B, device=dev())
    sp, sg = _t(batches[0][0]), _t(batches[0][1])
    out = {"_mvg_preds": sp, "views": V}
    eager.update(out, sg)                                        # (first call: library load, allocator)
    eager.reset()
    staged = [(_t(p), _t(l)) for p, l in batches]                # host-to-device copies of pageable memory synchronise: outside
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for p, l in staged:
            eager.update({"_mvg_preds": p, "views": V}, l)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    graphed = AngularErrorMeter(num_iter=2, dirs=6, capacity=3 * B, device=dev())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        graphed.update(out, sg)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.update(out, sg)
    graphed.reset()                                              # the warm-up update counted
    for p, l in staged:
        sp.copy_(p)
        sg.copy_(l)
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(graphed.record, eager.record) and torch.equal(graphed.err_out, eager.err_out)
    r = eager.record.cpu().numpy()
    assert (r[..., COUNT] == 3 * B).all() and np.abs(r[..., SUM] / (3 * want.sum(-1)) - 1).max() <= 1e-12


# ---------------------------------------------------------------- 7. model level
_MODEL = {}


def _model(compute=torch.float32):
    from rot_mvgaze_amd.model import FeatRotationSymm
    if compute not in _MODEL:
        sd = synth.make_state_dict(18, 0, 3, perturb_bn=True)
        m = FeatRotationSymm(backbone_depth=18, num_iter=3)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
        m.to(dev()).eval()
        m.compute_dtype = compute
        m.ensure_layout()
        _MODEL[compute] = m
    return _MODEL[compute]


def _inputs(B, V, hw=64, seed=1234):
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    inp = synth.make_inputs(B, V, seed, hw)
    img, hp, gt = (torch.from_numpy(inp[k]) for k in ("img", "head_pose", "gt_gaze"))
    imgs = [img[:, v].contiguous().to(dev()) for v in range(V)]
    rot = torch.stack([rotation_matrix_2d(hp[:, v].contiguous().to(dev())) for v in range(V)], dim=1).contiguous()
    return imgs, rot, gt.to(dev())


def _host(pred, gt):
    """trainer.py:128 / :192 on float64 arrays."""
    from rot_mvgaze_amd.geometry import angular_error
    return angular_error(pred.detach().cpu().numpy().astype(np.float64), gt.detach().cpu().numpy().astype(np.float64))


def test_model_level_two_views():
    from rot_mvgaze_amd.metrics import AngularErrorMeter
    m = _model()
    imgs, rot, gt = _inputs(3, 2)
    data = {"img_0": imgs[0], "img_1": imgs[1], "rot_0": rot[:, 0].contiguous(), "rot_1": rot[:, 1].contiguous(),
            "gt_gaze": gt[:, 0].contiguous(), "gt_gaze_1": gt[:, 1].contiguous()}
    with torch.no_grad():
        data = m(data)
    meter = AngularErrorMeter(num_iter=3, dirs=2, device=dev(), output_index=m._output_index)
    meter.update(data)
    c = meter.compute()
    want = float(np.mean(_host(data["pred_gaze"], data["gt_gaze"])))
    print(f"\nerror_gaze {c['error_gaze']:.12f} host {want:.12f}")
    assert want >= R.FLOOR_DEG and abs(c["error_gaze"] - want) <= R.PER_ELEMENT_BAR_DEG
    for i in range(3):
        for d, key in enumerate(("gt_gaze", "gt_gaze_1")):
            e = _host(data[f"iter_{i}"][f"pred_gaze_{d}"], data[key])
            assert e.min() >= R.FLOOR_DEG and abs(c["mean"][i, d] - e.mean()) <= R.PER_ELEMENT_BAR_DEG, (i, d)
            assert abs(c["max"][i, d] - e.max()) <= R.PER_ELEMENT_BAR_DEG and c["count"][i, d] == 3
    # the plain-tensor form is the same cell
    one = AngularErrorMeter(device=dev())
    one.update(data["pred_gaze"], data["gt_gaze"])
    assert one.compute()["error_gaze"] == c["mean"][m._output_index, 0]


def test_model_level_three_views():
    from rot_mvgaze_amd.metrics import AngularErrorMeter
    m = _model()
    imgs, rot, gt = _inputs(3, 3)
    with torch.no_grad():
        out = m.forward_multiview(imgs, rot)
    meter = AngularErrorMeter(num_iter=3, dirs=6, device=dev(), output_index=m._output_index)
    meter.update(out, gt)
    c = meter.compute()
    assert abs(c["error_gaze"] - float(np.mean(_host(out["pred_gaze"], gt[:, 0])))) <= R.PER_ELEMENT_BAR_DEG
    p = 0
    for a in range(3):
        for b in range(a + 1, 3):
            for i in range(3):
                for k, v in ((0, a), (1, b)):
                    e = _host(out["pairs"][(a, b)][f"iter_{i}"][f"pred_gaze_{k}"], gt[:, v])
                    assert e.min() >= R.FLOOR_DEG and abs(c["mean"][i, 2 * p + k] - e.mean()) <= R.PER_ELEMENT_BAR_DEG, (a, b, i, k)
            p += 1


def test_meter_inside_a_graphed_training_step():
    """GraphedStep's eager warm-up steps count (the capture pass runs nothing); after reset() every replay adds one batch."""
    from rot_mvgaze_amd.graph import GraphedStep
    from rot_mvgaze_amd.losses import MultiViewIterationLoss
    from rot_mvgaze_amd.metrics import AngularErrorMeter
    from rot_mvgaze_amd.model import MultiViewGaze
    from rot_mvgaze_amd.optim import Adam
    B, V = 2, 2
    m = MultiViewGaze(18, 3)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.make_state_dict(18, 0, 3).items()}, strict=True)
    m.to(dev()).train()
    imgs, rot, gt = _inputs(B, V, seed=77)
    crit = MultiViewIterationLoss(rel_weight=0.01, reference_decay=1.0, iter_decay=0.5)
    opt = Adam(m.parameters(), lr=1e-3, weight_decay=1e-6, capturable=True)
    meter = AngularErrorMeter(num_iter=3, dirs=2, capacity=8, device=dev())
    last = {}

    def step():
        m.zero_grad(set_to_none=True)
        out = m.forward_multiview(imgs, rot)
        meter.update(out, gt)
        last["preds"] = out["_mvg_preds"]
        loss = crit(out, gt)
        loss.backward()
        opt.step()
        return loss
    gs = GraphedStep(m, step, opt, warmup=2)
    assert (meter.compute()["count"] == 2 * B).all()             # the two warm-up steps
    meter.reset()
    for _ in range(2):
        gs.run()
    c, e = meter.compute(), meter.errors()
    assert (c["count"] == 2 * B).all() and e.shape == (3, 2, 2 * B)
    gt_dir = np.stack([gt[:, 0].cpu().numpy(), gt[:, 1].cpu().numpy()])
    want = R.oracle_cells(last["preds"].detach().cpu().numpy(), gt_dir)              # the static buffer holds the last replay's preds
    assert np.abs(e[..., B:].astype(np.float64) - want).max() <= _fp32_bar(want).max()


# ---------------------------------------------------------------- 8. session
@pytest.mark.parametrize("compute", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_session_hook(compute):
    from rot_mvgaze_amd import _lib
    from rot_mvgaze_amd.metrics import AngularErrorMeter
    from rot_mvgaze_amd.session import InferenceSession
    m = _model(compute)
    B, V = 2, 2
    imgs, rot, gt = _inputs(B, V)
    kw = dict(compute=torch.bfloat16) if compute == torch.bfloat16 else {}
    with InferenceSession(m, V, B, 64, 64, **kw) as plain:
        want = [o.clone() for o in plain.run(imgs, rot)]
        launches = plain.launches
    meter = AngularErrorMeter(num_iter=3, dirs=2, capacity=4, device=dev())
    with InferenceSession(m, V, B, 64, 64, meter=meter, **kw) as s:
        assert s.launches == launches + 1
        with pytest.raises(ValueError):
            s.run(imgs, rot)                                     # a session with a meter needs the labels
        out = s.empty_outputs()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            got = s.run(imgs, rot, out=out, gt=gt)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        # the record is a stand-alone mvg_gaze_error_update on those preds, bit for bit
        rec, eo = _record(3, 2), torch.empty(3, 2, 4, dtype=torch.float32, device=dev())
        _update(got[3], torch.stack([gt[:, 0], gt[:, 1]], 0).contiguous(), rec, eo, 4)
        assert torch.equal(meter.record, rec) and torch.equal(meter.err_out[..., :B], eo[..., :B])
        assert (meter.compute()["count"] == B).all()
        e = _host(got[3][m._output_index, 0], gt[:, 0])
        assert abs(meter.compute()["error_gaze"] - e.mean()) <= R.PER_ELEMENT_BAR_DEG
        # detached: the plain forward again, the record untouched
        before = meter.record.clone()
        _lib.check(_lib.lib().mvg_session_set_error_record(s._h, None, None, None, 0), "session_set_error_record")
        assert _lib.lib().mvg_session_launches(s._h) == launches
        s.meter = None
        again = s.run(imgs, rot)
        for a, b in zip(again, want):
            assert torch.equal(a, b)
        assert torch.equal(meter.record, before)
    with pytest.raises(ValueError):
        InferenceSession(m, V, B, 64, 64, meter=AngularErrorMeter(num_iter=3, dirs=6, device=dev()), **kw)
