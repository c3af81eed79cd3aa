"""model.split_frozen: frozen-BatchNorm training steps (model.train() + freeze_batchnorm) of the fp32 model on the split-operand
kernels.  ResNet-18, default variant, V = 2, B = 4, 64 px, synth.make_state_dict(..., perturb_bn=True) unless said otherwise.

accuracy    against the float64 oracle in eval mode (R.model_forward(..., training=False)) with the HIP forward's ReLU pattern
            imposed, at TOL = 1e-4 (loss, predictions) and GTOL = 2e-4 (every parameter gradient, max-norm relative) of
            tests/test_eval_backward_gpu.py - the bars tests/test_model_gpu.py holds both kernel families to in train mode.
call shape  sp, the row-window stem, training False, train_step True, every tape unit Family.SPLIT - this and the accuracy test's
            own call-shape assertion fail without the feature: the attribute is then inert and the call comes back with sp False.
range       gamma of one unit scaled and running_var of another shrunk until the float64 oracle's stored activations pass fp16's
            65 520 (checked on the CPU first, with the oracle's loss and gradients still finite): the step must still meet TOL and
            GTOL, and the units' slots show a scale 2^k < 1 (the slot holds 2^-k, as mvg_act_scales' slots do: a value above 1).
and         buffers bit-unchanged, run-to-run determinism, the train-mode publish order, the fine-tuning boundary (launch_spy of
            tests/test_finetune_gpu.py), no host synchronisation, a captured fine-tuning step (graph.GraphedStep) bit-equal to the
            eager one, ResNet-50 (V = 2, B = 2, 64 px) within TOL of the flag-off step of the same build.
Every figure is printed (`FROZEN-SPLIT ...`) before it is asserted.  Measured on an MI355X (profiles/frozen_split_errors.txt): loss
2.8e-07, predictions 8.2e-07, worst gradient 3.9e-06; with two activations at 1.1e6 and 2.0e6 (slots 2^8, 2^9): 2.6e-07, 9.3e-07,
3.2e-06; ResNet-50 against the flag-off step: loss 6.2e-07, predictions 1.4e-06."""
import numpy as np
import pytest
import torch

from rot_mvgaze_amd import synth
from test_eval_backward_gpu import GTOL, TOL, _grad_errors, _oracle_leaves, rel_close, rel_err
from test_finetune_gpu import BB, freeze, launch_spy
from test_frozen_bn_gpu import assert_buffers_equal, buffers, inputs, metrics, step
from test_model_gpu import _captured_masks

pytestmark = pytest.mark.gpu

OVER = 65520.0


def dev():
    return torch.device("cuda:0")


_SD = {}


def state(depth):
    if depth not in _SD:
        _SD[depth] = synth.make_state_dict(depth, 0, 3, perturb_bn=True)
    return _SD[depth]


def build(depth=18, flag=True, frozen=True, sd=None):
    from rot_mvgaze_amd.model import FeatRotationSymm
    m = FeatRotationSymm(backbone_depth=depth, num_iter=3)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in (sd or state(depth)).items()}, strict=True)
    m.to(dev()).train()
    m.freeze_batchnorm = frozen
    m.split_frozen = flag
    m._debug_keep_tapes = True            # assert_call_shape reads the tape's units
    return m


def assert_call_shape(m, depth=18):
    from rot_mvgaze_amd.backbone import Family
    call = m._backbone._last_call
    assert call.sp and call.stem_rw and not call.training and call.train_step, call._replace(wprep=None, act_sinv=None)
    units = m._last_backbone_tape["units"]
    assert len(units) == sum(1 for _ in m._backbone.spec.all_convs())
    assert all(u.family is Family.SPLIT and not u.trained for u in units)


def _against_the_oracle(m, sdn, batch, hw, seed, what):
    """One step of m against the float64 eval-mode oracle with m's ReLU pattern; returns the model's _act_sinv."""
    from oracle import restatement as R
    m._debug_keep_tapes = True
    data = m(inputs(batch, hw, seed=seed))
    assert_call_shape(m)
    masks = _captured_masks(m)
    loss = metrics()(data)
    loss.backward()
    sd, leaves = _oracle_leaves(sdn)
    inp = synth.make_inputs(batch, 2, seed, hw)
    img, hp, gt = (torch.from_numpy(inp[k]) for k in ("img", "head_pose", "gt_gaze"))
    od = {"img_0": img[:, 0].double(), "img_1": img[:, 1].double(),
          "rot_0": R.rotation_matrix_2d(hp[:, 0]).double(), "rot_1": R.rotation_matrix_2d(hp[:, 1]).double(),
          "gt_gaze": gt[:, 0], "gt_gaze_1": gt[:, 1]}
    od = R.model_forward(sd, od, 18, 3, False, masks)
    ol = R.iteration_loss(od)
    ol.backward()
    assert bool(torch.isfinite(ol)) and all(bool(torch.isfinite(v.grad).all()) for v in leaves.values() if v.grad is not None)
    errs = _grad_errors(m, leaves)
    print(f"FROZEN-SPLIT {what}: loss {rel_err(loss, ol.item()):.3e}, pred {rel_err(data['pred_gaze'], od['pred_gaze']):.3e} (bar {TOL}); "
          f"worst gradients (bar {GTOL}): " + ", ".join(f"{k} {e:.2e}" for e, k in errs[:4]))
    rel_close(loss, ol.item(), TOL, "loss")
    rel_close(data["pred_gaze"], od["pred_gaze"], TOL, "pred_gaze")
    assert len(errs) == len(leaves) - 2          # everything but the unused fc.weight / fc.bias
    assert errs[0][0] <= GTOL, "worst gradients (max-norm relative error): " + ", ".join(f"{k} {e:.2e}" for e, k in errs[:8])
    return {k: float(v) for k, v in m._backbone._act_sinv.items()}


def test_flagged_frozen_step_against_the_float64_oracle_and_its_call_shape():
    m = build()
    before = buffers(m)
    sinv = _against_the_oracle(m, state(18), 4, 64, 99, "r18 B4 64px")
    assert_buffers_equal(before, m)
    # every stored sp activation has a slot (the downsample branches' normalised maps are never stored): a power of two
    spec = m._backbone.spec
    stored = [c.name for c in spec.all_convs() if not any(b.downsample is c for b in spec.blocks)]
    assert sorted(sinv) == sorted(stored)
    assert all(v > 0 and np.log2(v) == int(np.log2(v)) for v in sinv.values()), sinv


def test_call_shape_of_a_flagged_frozen_step_and_the_flag_off_step_beside_it():
    data = inputs(4, 64)
    m = build()
    step(m, data)
    assert_call_shape(m)
    off = build(flag=False)
    step(off, data)
    call = off._backbone._last_call
    assert not call.sp and not call.stem_rw and not call.training and call.train_step
    # the flag is inert in eval() and in a train-mode step
    ev = build()
    ev.eval()
    step(ev, data)
    assert not ev._backbone._last_call.sp
    tr = build(frozen=False)
    step(tr, data)
    assert tr._backbone._last_call.training and tr._backbone._last_call.sp and tr._backbone._last_call.act_sinv is not None


def test_buffers_are_bit_unchanged_and_two_runs_give_the_same_bits():
    m = build()
    before = buffers(m)
    assert any(k.endswith("num_batches_tracked") for k in before)
    data = inputs(4, 64, seed=5)
    (l0, g0), (l1, g1) = step(m, data), step(m, data)
    assert_call_shape(m)
    assert torch.equal(l0, l1) and len(g0) > 60 and set(g0) == set(g1)
    for k, g in g0.items():
        assert torch.equal(g, g1[k]), k
    assert_buffers_equal(before, m)


def test_publish_order_is_the_train_mode_one():
    m = build(frozen=False)
    names = {id(p): k for k, p in m.named_parameters()}
    data = inputs(2, 64)

    def batches(frozen):
        m.freeze_batchnorm = frozen
        seen = []
        m._on_grads_ready = lambda ps: seen.append([names[id(p)] for p in ps])
        m.zero_grad(set_to_none=True)
        metrics()(m(dict(data))).backward()
        torch.cuda.synchronize()
        m._on_grads_ready = None
        return seen
    fr = batches(True)
    assert m._backbone._last_call.sp and not m._backbone._last_call.training
    tr = batches(False)
    assert len(fr) > 5 and fr == tr


# ---------------------------------------------------------------- range
RANGE_FACTOR = 3.0e5
RANGE_UP = (BB + "layer1.0.bn1", BB + "layer1.1.bn2")       # gamma and beta times the factor: a mid-block unit, a block's last unit
# ... and the BatchNorms that read those outputs through a conv take the factor into their running statistics (mean x F,
# variance x F^2), so that everything behind them - the predictions, the loss - stays as well conditioned as it was: the
# oracle is the same perturbed model either way, but a loss that is the sine of 1e7 radians could hold nobody to 1e-4
RANGE_ABSORB = (BB + "layer1.0.bn2", BB + "layer2.0.bn1", BB + "layer2.0.downsample.1")


def _range_state():
    sd = {k: np.array(v) for k, v in state(18).items()}
    for name in RANGE_UP:
        sd[name + ".weight"] = (sd[name + ".weight"] * RANGE_FACTOR).astype(np.float32)
        sd[name + ".bias"] = (sd[name + ".bias"] * RANGE_FACTOR).astype(np.float32)
    for name in RANGE_ABSORB:
        sd[name + ".running_mean"] = (sd[name + ".running_mean"] * RANGE_FACTOR).astype(np.float32)
        sd[name + ".running_var"] = (sd[name + ".running_var"] * RANGE_FACTOR ** 2).astype(np.float32)
    return sd


def test_range_activations_past_fp16_still_meet_the_bars():
    import torch.nn.functional as F
    from oracle import restatement as R
    from rot_mvgaze_amd.arch import backbone_spec
    sdn = _range_state()
    # on the CPU first: two of the float64 oracle's stored activations pass 65 520 - layer1.0.conv1's unit output and layer1.1's
    # block output - and nothing else does (that the oracle's loss and gradients are finite, _against_the_oracle asserts)
    sd, _ = _oracle_leaves(sdn)
    spec = backbone_spec(18)
    img = torch.from_numpy(synth.make_inputs(4, 2, 99, 64)["img"])
    peaks = {}
    with torch.no_grad():
        for v in range(2):
            trace = []
            R.backbone_forward(sd, img[:, v].double(), spec, False, trace)
            mid = F.relu(R._conv_bn(sd, trace[0], spec.blocks[0].convs[0], False))
            for name, t in [(spec.stem.name, trace[0]), (spec.blocks[0].convs[0].name, mid)] + \
                    [(blk.convs[-1].name, t) for blk, t in zip(spec.blocks, trace[1:])]:
                peaks[name] = max(peaks.get(name, 0.0), float(t.abs().max()))
    print("FROZEN-SPLIT range: the oracle's stored activations peak at " + ", ".join(f"{k[len(BB):]} {p:.3e}" for k, p in peaks.items()))
    over = sorted(k for k, p in peaks.items() if p > OVER)
    assert over == sorted([BB + "layer1.0.conv1", BB + "layer1.1.conv2"]) and all(np.isfinite(p) for p in peaks.values())
    m = build(sd=sdn)
    sinv = _against_the_oracle(m, sdn, 4, 64, 99, "range r18 B4 64px")
    print("FROZEN-SPLIT range: slots " + ", ".join(f"{k[len(BB):]} 2^{np.log2(v):.0f}" for k, v in sinv.items() if v != 1.0))
    for name in over:
        # the slot holds 2^-k; a value above 1 is a scale 2^k below 1: the tensor is stored below 2^15, not as inf
        assert sinv[name] > 1.0, (name, sinv[name], peaks[name])
        assert peaks[name] / sinv[name] < 2.0 ** 15
    assert sinv[spec.stem.name] == 1.0


# ---------------------------------------------------------------- fine-tuning
def below_layer4(name):
    return name.startswith(BB) and ".fc." not in name and ".layer4." not in name


def test_fine_tuning_boundary_is_silent_below_it_and_produces_the_flag_off_gradients():
    data = inputs(4, 64)
    off = build(flag=False)
    frozen = freeze(off, below_layer4)
    _, ref = step(off, data)
    m = build()
    assert freeze(m, below_layer4) == frozen
    with launch_spy() as calls:
        _, grads = step(m, data)
    assert_call_shape(m)
    assert calls and [c for c in calls if below_layer4(c[1])] == []
    assert [c for c in calls if c[0] == "_dgrad" and c[1] in (BB + "layer4.0.conv1", BB + "layer4.0.downsample.0")] == []
    assert ("_wgrad", BB + "layer4.0.conv1") in calls and ("_wgrad", BB + "layer4.0.downsample.0") in calls
    assert set(grads) == set(ref) and not (set(grads) & set(frozen))
    worst = max((rel_err(g, ref[k]), k) for k, g in grads.items())
    # (a figure, no bar: the two kernel families take a handful of boundary ReLU decisions differently)
    print(f"FROZEN-SPLIT boundary: worst gradient against the flag-off step {worst[0]:.3e} ({worst[1]})")


def test_flagged_frozen_step_does_not_synchronise_the_host():
    from rot_mvgaze_amd.optim import Adam
    m = build()
    crit = metrics()
    opt = Adam(m.parameters(), lr=1e-4, weight_decay=1e-6)
    d = inputs(4, 64)

    def one():
        opt.zero_grad()
        crit(m(dict(d))).backward()
        opt.step()
    one()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        one()
        one()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert m._backbone._last_call.sp and not m._backbone._last_call.training


def test_captured_fine_tuning_step_replays_the_eager_step_bit_for_bit():
    """test_graph_finetune_gpu's scheme: stem, layer1 and layer2 frozen, two parameter groups, frozen BatchNorm - with the flag."""
    from rot_mvgaze_amd.graph import GraphedStep
    from test_graph_finetune_gpu import _same_state, _setup
    m1, o1, s1 = _setup(freeze_bn=True)
    m1.split_frozen = True
    bufs = buffers(m1)
    eager = [float(s1().item()) for _ in range(3)]
    assert m1._backbone._last_call.sp and not m1._backbone._last_call.training and m1._backbone._last_call.stem_rw
    m2, o2, s2 = _setup(freeze_bn=True)
    m2.split_frozen = True
    gs = GraphedStep(m2, s2, o2, warmup=2)
    graph = [float(gs.run().item())]
    assert graph == eager[2:], (graph, eager)
    _same_state(m1, o1, m2, o2)
    assert_buffers_equal(bufs, m1)
    assert_buffers_equal(bufs, m2)


def test_resnet50_runs_every_unit_on_the_split_kernels_and_agrees_with_the_flag_off_step():
    """V = 2, B = 2, 64 px: loss and predictions of the flagged step within TOL of the flag-off step of the same build."""
    from rot_mvgaze_amd.backbone import Family
    data = inputs(2, 64)
    off, on = build(50, flag=False), build(50)
    on._debug_keep_tapes = True
    d_off, d_on = off(dict(data)), on(dict(data))
    l_off, l_on = metrics()(d_off), metrics()(d_on)
    units = on._last_backbone_tape["units"]
    assert len(units) == 53 and all(u.family is Family.SPLIT and not u.trained for u in units)
    call = on._backbone._last_call
    assert call.sp and call.stem_rw and not call.training and call.train_step
    assert not off._backbone._last_call.sp
    l_on.backward()
    torch.cuda.synchronize()
    print(f"FROZEN-SPLIT r50 B2 64px against the flag-off step: loss {rel_err(l_on, l_off.item()):.3e}, "
          f"pred {rel_err(d_on['pred_gaze'], d_off['pred_gaze']):.3e} (bar {TOL})")
    rel_close(l_on, l_off.item(), TOL, "loss")
    rel_close(d_on["pred_gaze"], d_off["pred_gaze"], TOL, "pred_gaze")
    assert all(bool(torch.isfinite(p.grad).all()) for p in on.parameters() if p.grad is not None)
