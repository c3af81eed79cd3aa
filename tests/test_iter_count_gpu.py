"""Iteration counts other than 3 and IterationLoss's additional_decay, on every path that depends on them.

The rest of the suite builds the model with num_iter = 3 and the loss with additional_decay = None; the code is written for any
count.  Here: the loss modules' weight tables (both branches of IterationLoss, MultiViewIterationLoss) against fixtures written
by the reference's own IterationLoss and against the oracle; the fusion head alone at I in {1, 2, 4, 5, 6} on its fp32, split and
bf16 ("mixed") Linears against the fp64 oracle with the forward's ReLU patterns (tests/fusion_head_harness.py, the harness of
tests/test_fusion_split_gpu.py); the whole model at I in {1, 4} against the oracle; the inference session at I in {1, 2, 5}.
The parametrisations that other files already own carry their I = 2 cases themselves (test_model_gpu.py: the reference fixture,
the strict backward, one multi-view case; test_bf16_gpu.py; test_graph_gpu.py).

No bar is new.  Each is imported from, or restated next to the name of, the test that holds the same quantity at I = 3, and every
comparison prints its figure (a line starting ITER-COUNT; pytest -s shows them) before it asserts.

The split head serves I <= 5 (11 scale slots per iteration plus 2 in a 64-slot arena); from 6 it steps aside to the fp32 Linears
(FusionHead.split_serves), as the backbone's split path does at 2 GiB per view.

Measured on an MI355X (profiles/iter_count_errors.txt), smallest .. largest over the cases; no bar was fitted to them:
head alone, relative L2 against fp64 under the 2e-5 bar - fp32 Linears 1.1e-08 .. 4.7e-07 (I = 1, 2, 4), split Linears
7.5e-08 .. 2.4e-06 (I = 1, 2, 4, 5, share_weights, ignore_rotmat; at I = 3 the same harness measures 3.5e-08 .. 4.2e-06), I = 6
stepping aside 3.3e-08 .. 9.2e-07; bf16 Linears features at most 1.2e-03 (bar 6e-3), predictions 5.5e-04 (3e-2), gradients
5.6e-03 (2e-1); IterationLoss on the reference's 24 rows loss at most 2.8e-07 (1e-5), d pred 2.9e-06 (1e-4), fused against
generic 1.1e-07 / 7.4e-08 (1e-6); whole model at I = 1 / 4 predictions 4.8e-06 / 7.2e-06 (1e-4), gradients at most 8.1e-06
relative L2 (3e-2); every session comparison bit-equal; the session's meter 2.1e-14 deg from the host metric (1e-8)."""
import os

import numpy as np
import pytest
import torch

import fusion_head_harness as H
import gaze_error_ref as GR
import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd import synth
from test_bf16_gpu import BF16_GRAD_L2, BF16_PRED_TOL, OUT_RTOL
from test_fusion_split_gpu import BLOCK_BARS
from test_model_gpu import TOL, build, check_outputs, inputs, l2_bound, l2_close, metrics, rel_close

pytestmark = pytest.mark.gpu

# tests/test_kernels_gpu.py::test_geometry_and_loss_golden, the loss kernel against the reference's fixture
LOSS_RTOL = 1e-5                # np.testing.assert_allclose(loss, ref, rtol=1e-5)
DPRED_RTOL = 1e-4               # np.testing.assert_allclose(dpred, ref, rtol=1e-4, atol=1e-4 * max |ref|)
# tests/test_model_gpu.py::test_against_oracle_and_generic_loss_path, generic against fused: rel_close(..., 1e-6)
BRANCHES_TOL = 1e-6
# the bf16 ("mixed") Linears of the block against the bf16-storage oracle (tests/test_bf16_gpu.py): fp32 outputs of bf16
# products at the bar of a bf16-rounded output (OUT_RTOL), predictions at BF16_PRED_TOL, gradients at BF16_GRAD_L2 (relative L2)
MIXED_BARS = {"feat": ("max-norm", OUT_RTOL), "pred": ("max-norm", BF16_PRED_TOL), "dimg": ("rel-L2", BF16_GRAD_L2),
              "grad": ("rel-L2", BF16_GRAD_L2)}


def dev():
    return torch.device("cuda:0")


def say(line):
    print("ITER-COUNT " + line)


# ---------------------------------------------------------------- 1. IterationLoss, both branches, on the reference's rows
_FIXTURE = {}


def _iteration_loss_fixture(golden_dir):
    if not _FIXTURE:
        g = np.load(os.path.join(golden_dir, "iteration_loss_decay.npz"))
        _FIXTURE["g"] = g
        _FIXTURE["cases"] = [(i, int(n), float(d), None if a < 0 else float(a)) for i, (n, d, a) in enumerate(g["cases"])]
    return _FIXTURE["g"], _FIXTURE["cases"]


def _run_iteration_loss(preds_np, gt_np, n, d, a, fused):
    """IterationLoss(StereoL1Loss(0.01, 1.0), d, a) on a prediction dict built from preds [n,2,B,2]; `fused`: the dict carries
    the stacked `_mvg_preds` (one launch for every iteration), otherwise the generic per-iteration branch runs."""
    from rot_mvgaze_amd.losses import IterationLoss, StereoL1Loss
    p = torch.from_numpy(preds_np[:n].copy()).to(dev()).requires_grad_(True)
    gt = torch.from_numpy(gt_np).to(dev())
    data = {"num_iter": n, "gt_gaze": gt[0].contiguous(), "gt_gaze_1": gt[1].contiguous()}
    for it in range(n):
        data[f"iter_{it}"] = {"pred_gaze_0": p[it, 0], "pred_gaze_1": p[it, 1]}
    if fused:
        data["_mvg_preds"] = p
    crit = IterationLoss(StereoL1Loss(rel_weight=0.01, reference_decay=1.0, distance_metric="angular_error", pred_gaze_key="pred_gaze"),
                         iter_decay=d, additional_decay=a)
    loss = crit(data)
    assert (type(loss.grad_fn).__name__ == "_FusedIterLossFnBackward") == fused, type(loss.grad_fn).__name__      # the branch that ran
    loss.backward()
    return float(loss.item()), p.grad.detach().cpu().numpy()


def test_iteration_loss_both_branches_against_the_reference_rows(golden_dir):
    """Every row of iteration_loss_decay.npz (the reference's IterationLoss: counts 1..4, iter_decay 0.5 / 1.0, additional_decay
    None / 0.25 / 0.0) through the fused and the generic branch: loss and d loss / d pred of every iteration against the fixture
    at the loss kernel's own bars, the branches against each other at 1e-6, and with additional_decay = 0.0 the last iteration's
    gradient rows exactly zero."""
    g, cases = _iteration_loss_fixture(golden_dir)
    assert len(cases) == 24
    worst = {"loss": [], "dpred": [], "branch loss": [], "branch dpred": []}
    for idx, n, d, a in cases:
        ref_loss, ref_d = float(g[f"loss_{idx}"]), g[f"dpred_{idx}"]
        out = {}
        for fused in (True, False):
            loss, dp = _run_iteration_loss(g["pred"], g["gt"], n, d, a, fused)
            out[fused] = (loss, dp)
            assert dp.shape == ref_d.shape == (n, 2, 5, 2)
            worst["loss"].append((abs(loss - ref_loss) / max(abs(ref_loss), 1e-30) if ref_loss else abs(loss), (n, d, a, fused)))
            worst["dpred"].append((float(np.abs(dp - ref_d).max() / max(np.abs(ref_d).max(), 1e-30)) if ref_d.any() else float(np.abs(dp).max()),
                                   (n, d, a, fused)))
            if a == 0.0:
                assert not dp[n - 1].any(), (n, d, a, fused)
                assert n == 1 or np.abs(dp[:n - 1]).min() > 0
        (lf, df), (lg, dg) = out[True], out[False]
        worst["branch loss"].append((abs(lg - lf) / max(abs(lf), 1e-30) if lf else abs(lg), (n, d, a)))
        worst["branch dpred"].append((float(np.abs(dg - df).max() / max(np.abs(df).max(), 1e-30)) if df.any() else float(np.abs(dg).max()), (n, d, a)))
    bars = {"loss": LOSS_RTOL, "dpred": DPRED_RTOL, "branch loss": BRANCHES_TOL, "branch dpred": BRANCHES_TOL}
    for k, v in worst.items():
        v.sort(key=lambda t: t[0])
        say(f"IterationLoss on the reference's rows, {k}: relative {v[0][0]:.3e} .. {v[-1][0]:.3e} over {len(v)} comparisons "
            f"(largest at {v[-1][1]}; bar {bars[k]:.1e})")
    for k, v in worst.items():
        assert v[-1][0] <= bars[k], (k, v[-1])


def _mv_case(I, V, B, seed):
    """Synthetic stacked predictions [I, D, B, 2] and labels [B, V, 2], every row 0.05 .. 0.6 rad per component off its label."""
    from rot_mvgaze_amd.heads import directed_pairs
    rng = np.random.default_rng(seed)
    vi, _ = directed_pairs(V)
    gt = rng.uniform(-1, 1, size=(B, V, 2)).astype(np.float32)
    off = rng.uniform(0.05, 0.6, size=(I, len(vi), B, 2)) * rng.choice([-1.0, 1.0], size=(I, len(vi), B, 2))
    preds = (np.stack([gt[:, v] for v in vi], 0)[None] + off).astype(np.float32)
    return preds, gt, vi


@pytest.mark.parametrize("I", [1, 2, 4])
def test_multiview_iteration_loss_three_views_against_the_oracle(I):
    """MultiViewIterationLoss at V = 3 (six directed pairs) with and without additional_decay against oracle.multiview_loss (the
    mean over pairs of the two-view iteration loss): loss and d loss / d pred at the loss kernel's bars."""
    from oracle import restatement as R
    from rot_mvgaze_amd.losses import MultiViewIterationLoss
    V, B = 3, 5
    preds_np, gt_np, vi = _mv_case(I, V, B, 40 + I)
    for a in (None, 0.25, 0.0):
        p = torch.from_numpy(preds_np).to(dev()).requires_grad_(True)
        loss = MultiViewIterationLoss(rel_weight=0.01, reference_decay=1.0, iter_decay=0.5, additional_decay=a)(
            {"_mvg_preds": p, "views": V}, torch.from_numpy(gt_np).to(dev()))
        loss.backward()
        po = torch.from_numpy(preds_np).requires_grad_(True)
        pairs = {}
        for k, pr in enumerate(R.view_pairs(V)):
            assert (vi[2 * k], vi[2 * k + 1]) == pr
            pairs[pr] = {"num_iter": I, **{f"iter_{it}": {"pred_gaze_0": po[it, 2 * k], "pred_gaze_1": po[it, 2 * k + 1]} for it in range(I)}}
        ol = R.multiview_loss({"pairs": pairs}, torch.from_numpy(gt_np), 0.5, 0.01, 1.0, a)
        ol.backward()
        el = abs(loss.item() - ol.item()) / abs(ol.item()) if ol.item() else abs(loss.item())
        ref = po.grad.numpy()
        got = p.grad.cpu().numpy()                          # (I = 1 with additional_decay = 0.0: the reference gradient is all zeros)
        ed = float(np.abs(got - ref).max() / np.abs(ref).max()) if ref.any() else float(np.abs(got).max())
        say(f"MultiViewIterationLoss V=3 I={I} additional_decay={a}: loss {el:.3e} (bar {LOSS_RTOL:.1e}), dpred {ed:.3e} of max |ref| (bar {DPRED_RTOL:.1e})")
        assert el <= LOSS_RTOL and ed <= DPRED_RTOL, (I, a, el, ed)
        if a == 0.0:
            assert not p.grad[I - 1].any()


def test_loss_launch_at_exactly_512_cells_against_the_oracle():
    """mvg_gaze_angular_loss_multi carries its weights by value in a float[512]: 8 iterations x 64 directions fill it to the last
    cell (513 is refused before any launch: tests/test_gaze_error_cpu.py).  Every cell has its own weight; loss and gradient
    against the oracle's per-cell angular loss at the loss kernel's bars."""
    from oracle import restatement as R
    from rot_mvgaze_amd import ops
    I, D, B = 8, 64, 3
    rng = np.random.default_rng(512)
    gt = rng.uniform(-1, 1, size=(D, B, 2)).astype(np.float32)
    preds = (gt[None] + rng.uniform(0.05, 0.6, size=(I, D, B, 2)) * rng.choice([-1.0, 1.0], size=(I, D, B, 2))).astype(np.float32)
    w = rng.uniform(0.1, 1.0, size=I * D)
    p = torch.from_numpy(preds).to(dev())
    loss, dpred = torch.zeros(1, device=dev()), torch.full((I, D, B, 2), float("nan"), device=dev())
    ops.gaze_angular_loss_multi(p, torch.from_numpy(gt).to(dev()), I, D, B, list(w), loss, dpred)
    po = torch.from_numpy(preds).requires_grad_(True)
    total = 0
    for it in range(I):
        for d in range(D):
            total = total + float(np.float32(w[it * D + d])) * R.gaze_angular_loss(po[it, d], torch.from_numpy(gt[d]))
    total.backward()
    el = abs(loss.item() - total.item()) / abs(total.item())
    ref = po.grad.numpy()
    ed = float(np.abs(dpred.cpu().numpy() - ref).max() / np.abs(ref).max())
    say(f"loss launch at 8 x 64 = 512 cells: loss {el:.3e} (bar {LOSS_RTOL:.1e}), dpred {ed:.3e} of max |ref| (bar {DPRED_RTOL:.1e})")
    assert el <= LOSS_RTOL and ed <= DPRED_RTOL
    last = dpred[I - 1, D - 1].cpu().numpy()                      # the 512th weight reached the kernel
    assert np.abs(last - ref[I - 1, D - 1]).max() <= DPRED_RTOL * np.abs(ref).max() and np.abs(last).min() > 0


# ---------------------------------------------------------------- 2. the fusion head alone
HEAD_CASES = [
    # id, V, B, I, variant, head.split, head.mixed, tape mode
    ("fp32_V2_B5_I1", 2, 5, 1, None, True, False, "fp32"), ("fp32_V2_B5_I2", 2, 5, 2, None, True, False, "fp32"),
    ("fp32_V2_B5_I4", 2, 5, 4, None, True, False, "fp32"), ("fp32_V3_B4_I2", 3, 4, 2, None, True, False, "fp32"),
    ("split_V4_B96_I1", 4, 96, 1, None, True, False, "split"), ("split_V4_B96_I2", 4, 96, 2, None, True, False, "split"),
    ("split_V4_B96_I4", 4, 96, 4, None, True, False, "split"),
    ("split_V4_B96_I5", 4, 96, 5, None, True, False, "split"),                 # the last count the slot arena serves
    ("split_share_weights_V4_B96_I4", 4, 96, 4, {"share_weights": True}, True, False, "split"),   # gradients summed over four iterations
    ("split_ignore_rotmat_V4_B96_I1", 4, 96, 1, {"ignore_rotmat": True}, True, False, "split"),
    ("split_steps_aside_V4_B96_I6", 4, 96, 6, None, True, False, "fp32"),     # 1152 rows, split asked for: the fp32 Linears serve it
    ("mixed_V2_B5_I2", 2, 5, 2, None, False, True, "mixed"), ("mixed_V2_B5_I4", 2, 5, 4, None, False, True, "mixed"),
]


@pytest.mark.parametrize("name,V,B,I,variant,split,mixed,mode", HEAD_CASES, ids=[c[0] for c in HEAD_CASES])
def test_fusion_head_at_other_iteration_counts_against_the_fp64_oracle(name, V, B, I, variant, split, mixed, mode):
    """The fusion head alone (ResNet-18 widths): features, predictions, d / d img_feat and every parameter gradient of each of the
    I iterations against the fp64 oracle with the forward's ReLU patterns.  fp32 and split paths: the 2e-5 relative L2 of
    tests/test_fusion_split_gpu.py (same harness); bf16 Linears: the bf16-storage oracle at test_bf16_gpu.py's bars."""
    from oracle import restatement as R
    from rot_mvgaze_amd.heads import FusionHead, SPLIT_MIN_ROWS
    run = H.run_head(18, V, B, I, variant_kw=variant, seed=5 + I, split=split, mixed=mixed)
    rows = V * (V - 1) * B
    assert run["tape"]["mode"] == mode, run["tape"]["mode"]
    if mode == "split":
        assert rows >= SPLIT_MIN_ROWS and FusionHead.split_serves(I) and "st" in run["tape"]
    if name.startswith("split_steps_aside"):
        assert rows >= SPLIT_MIN_ROWS and not FusionHead.split_serves(I) and FusionHead.split_serves(I - 1) and "st" not in run["tape"]
    assert run["preds"].shape == (I, V * (V - 1), B, 2) and run["feats"].shape[:3] == (I, V * (V - 1), B)
    assert torch.isfinite(run["feats"]).all() and torch.isfinite(run["preds"]).all()
    H.compare_with_oracle(run, f"head {name}", MIXED_BARS if mixed else BLOCK_BARS, R.bf16_round if mixed else None)


# ---------------------------------------------------------------- 3. the whole model against the oracle
def _oracle_step(I, batch, hw, seed, training, loss=True):
    from oracle import restatement as R
    sd = {k: torch.from_numpy(np.array(v)) for k, v in synth.make_state_dict(18, 0, I, perturb_bn=True).items()}
    leaves = {k: v.requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and "running" not in k} if loss else {}
    inp = synth.make_inputs(batch, 2, seed, hw)
    img, hp, gt = (torch.from_numpy(inp[k]) for k in ("img", "head_pose", "gt_gaze"))
    od = {"img_0": img[:, 0].contiguous(), "img_1": img[:, 1].contiguous(), "rot_0": R.rotation_matrix_2d(hp[:, 0]),
          "rot_1": R.rotation_matrix_2d(hp[:, 1]), "gt_gaze": gt[:, 0], "gt_gaze_1": gt[:, 1]}
    if not loss:
        with torch.no_grad():
            return R.model_forward(sd, od, 18, I, training), None, sd, leaves
    od = R.model_forward(sd, od, 18, I, training)
    ol = R.iteration_loss(od)
    ol.backward()
    return od, ol, sd, leaves


def _as_fixture(od, I, prefix):
    g = {f"{prefix}.{k}": od[k].detach().numpy() for k in ("img_feat_0", "img_feat_1", "initial_rot_feat_0", "initial_rot_feat_1", "pred_gaze")}
    for i in range(I):
        for k in ("feat_0", "feat_1", "pred_gaze_0", "pred_gaze_1"):
            g[f"{prefix}.iter_{i}.{k}"] = od[f"iter_{i}"][k].detach().numpy()
    return g


@pytest.mark.parametrize("I", [1, 4])
def test_whole_model_against_the_oracle(I):
    """FeatRotationSymm(18, num_iter=I) on the shapes of the reference fixture (V = 2, B = 3, 64 x 64) against the oracle at
    num_iter = I: eval outputs, then one training step - outputs, loss, every parameter gradient, the running statistics - at
    the bars test_model_gpu.py holds against the I = 3 fixture and oracle (TOL, FTOL, l2_bound)."""
    batch, hw = 3, 64
    m = build(18, train=False, num_iter=I)
    with torch.no_grad():
        data = m(inputs(batch, hw))
    assert data["num_iter"] == I and data["pred_gaze"] is data[f"iter_{I - 1}"]["pred_gaze_0"] and m._output_index == I - 1
    assert data["_mvg_preds"].shape == (I, 2, batch, 2)
    od, _, _, _ = _oracle_step(I, batch, hw, 1234, False, loss=False)
    assert od["pred_gaze"] is od[f"iter_{I - 1}"]["pred_gaze_0"]
    check_outputs(data, _as_fixture(od, I, "eval"), "eval", TOL, I)
    e = max(float((data[f"iter_{i}"][k].cpu() - od[f"iter_{i}"][k]).abs().max() / od[f"iter_{i}"][k].abs().max())
            for i in range(I) for k in ("pred_gaze_0", "pred_gaze_1"))
    say(f"whole model I={I} eval, predictions vs oracle: max-norm {e:.3e} (bar {TOL:.1e})")
    m = build(18, train=True, num_iter=I)
    data = m(inputs(batch, hw))
    assert data["num_iter"] == I and data["pred_gaze"] is data[f"iter_{I - 1}"]["pred_gaze_0"]
    loss = metrics()(data)
    loss.backward()
    od, ol, sd, leaves = _oracle_step(I, batch, hw, 1234, True)
    check_outputs(data, _as_fixture(od, I, "train"), "train", TOL, I)
    e = max(float((data[f"iter_{i}"][k].detach().cpu() - od[f"iter_{i}"][k].detach()).abs().max() / od[f"iter_{i}"][k].detach().abs().max())
            for i in range(I) for k in ("pred_gaze_0", "pred_gaze_1"))
    say(f"whole model I={I} train, predictions vs oracle: max-norm {e:.3e} (bar {TOL:.1e}); loss "
        f"{abs(loss.item() - ol.item()) / abs(ol.item()):.3e} (bar {TOL:.1e})")
    rel_close(loss, ol.item(), TOL, "loss")
    errs = []
    for k, p in m.named_parameters():
        if leaves[k].grad is None:
            assert p.grad is None, k
            continue
        got, ref = (p.grad.contiguous() if p.grad.dim() == 4 else p.grad).detach().cpu().double().numpy(), leaves[k].grad.numpy()
        errs.append((float(np.linalg.norm((got - ref).ravel()) / (np.linalg.norm(ref.ravel()) + 1e-30)), k))
    errs.sort()
    bound = l2_bound(18, batch, hw)
    say(f"whole model I={I} train, parameter gradients vs oracle: rel-L2 {errs[0][0]:.3e} .. {errs[-1][0]:.3e} over {len(errs)} tensors "
        f"(largest at {errs[-1][1]}; bar {bound:.1e})")
    assert len(errs) == len(leaves) - 2
    for k, p in m.named_parameters():
        if leaves[k].grad is not None:
            l2_close(p.grad.contiguous() if p.grad.dim() == 4 else p.grad, leaves[k].grad.numpy(), bound, "grad " + k)
    msd = m.state_dict()
    for k in ("_feat_extractor.0.bn1", "_feat_extractor.0.layer1.0.bn2", "_feat_extractor.0.layer2.0.downsample.1", "_feat_extractor.0.layer4.1.bn1"):
        rel_close(msd[k + ".running_mean"], sd[k + ".running_mean"].detach().numpy(), TOL, k + ".running_mean")
        rel_close(msd[k + ".running_var"], sd[k + ".running_var"].detach().numpy(), TOL, k + ".running_var")
        assert int(msd[k + ".num_batches_tracked"]) == int(sd[k + ".num_batches_tracked"]) == 2


# ---------------------------------------------------------------- 4. the inference session
_SESSION_MODELS = {}


def _session_model(I, form):
    """One eval-mode ResNet-18 per (count, form): 'fp32mfma' (MVG_SPLIT=0's kernels), 'split' (the default fp32 model), 'bf16'."""
    from rot_mvgaze_amd.model import FeatRotationSymm
    if (I, form) not in _SESSION_MODELS:
        sd = synth.make_state_dict(18, 0, I, perturb_bn=True)
        m = FeatRotationSymm(18, I)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
        m.to(dev()).eval()
        if form == "bf16":
            m.compute_dtype = torch.bfloat16
        m.ensure_layout()
        if form == "fp32mfma":
            m._backbone.split = False
        _SESSION_MODELS[(I, form)] = m
    return _SESSION_MODELS[(I, form)]


def _session_inputs(B, V, hw=64, seed=1234):
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    inp = synth.make_inputs(B, V, seed, hw)
    img, hp, gt = (torch.from_numpy(inp[k]) for k in ("img", "head_pose", "gt_gaze"))
    imgs = [img[:, v].contiguous().to(dev()) for v in range(V)]
    rot = torch.stack([rotation_matrix_2d(hp[:, v].contiguous().to(dev())) for v in range(V)], dim=1).contiguous()
    return imgs, rot, gt.to(dev())


def _session_against_the_module(I, form, V, B):
    """tests/test_session_gpu.py's and tests/test_session_bf16_gpu.py's comparison: torch.equal on all four outputs."""
    from rot_mvgaze_amd.session import InferenceSession
    m = _session_model(I, form)
    imgs, rot, _ = _session_inputs(B, V)
    with torch.no_grad():
        want = [o.detach().clone() for o in m.run_views(imgs, rot)]
    assert (m._head.mixed, m._backbone._split_now if form != "bf16" else False) == (form == "bf16", form == "split")
    D = V * (V - 1)
    kw = dict(compute=torch.bfloat16) if form == "bf16" else {}
    with InferenceSession(m, V, B, 64, 64, **kw) as s:
        got = s.run(imgs, rot)
        assert got[2].shape == (I, D, B, 3, 512) and got[3].shape == (I, D, B, 2)
        worst = 0.0
        for n, a, b in zip(("img_feat", "lifted", "feats", "preds"), got, want):
            assert a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.isfinite(b).all(), n
            worst = max(worst, (a - b).abs().max().item())
        say(f"session {form} I={I} V={V} B={B}: max |session - module| over the four outputs {worst:.1e} (torch.equal)")
        for n, a, b in zip(("img_feat", "lifted", "feats", "preds"), got, want):
            assert torch.equal(a, b), f"{n}: max |diff| {(a - b).abs().max().item():.3e}"
        return s.launches


@pytest.mark.parametrize("form", ["fp32mfma", "split", "bf16"])
@pytest.mark.parametrize("I", [1, 2, 5])
def test_session_at_other_iteration_counts_matches_the_module(I, form):
    _session_against_the_module(I, form, 2, 2)


def test_session_split_head_at_five_iterations():
    """1032 fusion rows: the session's head runs on the split Linears, at the last count their slot arena serves (6 is refused in
    words: tests/test_session_cpu.py)."""
    a = _session_against_the_module(5, "split", 4, 86)
    b = _session_against_the_module(5, "split", 4, 85)            # 1020 rows: the generated-input fp32-MFMA Linears
    assert a != b


def test_session_meter_at_two_iterations():
    """AngularErrorMeter(num_iter=2, dirs=2) attached to a session of a two-iteration model: the record is the stand-alone
    update on the session's predictions bit for bit, and every cell's mean is the host float64 metric's (tests/test_gaze_error_gpu.py)."""
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd.geometry import angular_error
    from rot_mvgaze_amd.metrics import AngularErrorMeter
    from rot_mvgaze_amd.session import InferenceSession
    I, V, B = 2, 2, 2
    m = _session_model(I, "split")
    imgs, rot, gt = _session_inputs(B, V)
    with InferenceSession(m, V, B, 64, 64) as plain:
        want = [o.clone() for o in plain.run(imgs, rot)]
        launches = plain.launches
    meter = AngularErrorMeter(num_iter=I, dirs=2, capacity=4, device=dev())
    with InferenceSession(m, V, B, 64, 64, meter=meter) as s:
        assert s.launches == launches + 1
        got = s.run(imgs, rot, out=s.empty_outputs(), gt=gt)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        rec = torch.zeros(I, 2, 5, dtype=torch.float64, device=dev())
        eo = torch.empty(I, 2, 4, dtype=torch.float32, device=dev())
        ops.gaze_error_update(got[3], torch.stack([gt[:, 0], gt[:, 1]], 0).contiguous(), I, 2, B, rec, eo, 4)
        assert torch.equal(meter.record, rec) and torch.equal(meter.err_out[..., :B], eo[..., :B])
        c = meter.compute()
        assert c["count"].shape == (I, 2) and (c["count"] == B).all()
        worst = 0.0
        for i in range(I):
            for d in range(2):
                e = angular_error(got[3][i, d].cpu().numpy().astype(np.float64), gt[:, d].cpu().numpy().astype(np.float64))
                assert e.min() >= GR.FLOOR_DEG
                worst = max(worst, abs(c["mean"][i, d] - e.mean()), abs(c["max"][i, d] - e.max()))
        e = angular_error(got[3][m._output_index, 0].cpu().numpy().astype(np.float64), gt[:, 0].cpu().numpy().astype(np.float64))
        worst = max(worst, abs(c["error_gaze"] - e.mean()))
        say(f"session meter I=2: largest |meter - host float64 metric| over the cells' mean and max {worst:.3e} deg (bar {GR.PER_ELEMENT_BAR_DEG:.1e})")
        assert m._output_index == I - 1 and worst <= GR.PER_ELEMENT_BAR_DEG
    with pytest.raises(ValueError):
        InferenceSession(m, V, B, 64, 64, meter=AngularErrorMeter(num_iter=3, dirs=2, device=dev()))
