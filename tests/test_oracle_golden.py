"""The CPU oracle (oracle/restatement.py) against fixtures generated from the reference's own
Python (tests/golden/make_golden.py).  CPU-only; this is what pins the oracle."""
import json
import os

import numpy as np
import pytest
import torch

import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd import synth
from oracle import restatement as R

torch.set_num_threads(8)


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def test_geometry_known_answers(golden_dir):
    g = _load(golden_dir, "geometry_loss.npz")
    hp = torch.from_numpy(g["hp"])
    np.testing.assert_allclose(R.rotation_matrix_2d(hp).numpy(), g["R"], rtol=0, atol=1e-7)
    np.testing.assert_array_equal(R.rotation_matrix_2d(hp, inverse=True).numpy(),
                                  R.rotation_matrix_2d(hp).transpose(1, 2).numpy())
    np.testing.assert_allclose(R.rotation_matrix_2d(hp, inverse=True).numpy(), g["R_inv"], atol=1e-7)
    np.testing.assert_allclose(R.rotation_matrix_2d(hp[0]).numpy(), g["R_1d"], atol=1e-7)
    np.testing.assert_allclose(R.pitchyaw_to_vector(hp).numpy(), g["vec"], atol=1e-7)
    # SURVEY §8(a) A1 known answer, hp = (0.1, 0.2)
    np.testing.assert_allclose(g["R"][0], [[0.98006660, -0.01983384, 0.19767681],
                                           [0.0, 0.99500418, 0.09983342],
                                           [-0.19866933, -0.09784340, 0.97517037]], atol=1e-7)
    # R @ e_z == pitchyaw_to_vector(hp)  (same convention for head pose and gaze)
    np.testing.assert_allclose(g["R"][:, :, 2], g["vec"], atol=1e-6)


def test_loss_known_answers(golden_dir):
    g = _load(golden_dir, "geometry_loss.npz")
    pred = torch.from_numpy(g["loss_pred"]).requires_grad_(True)
    gt = torch.from_numpy(g["loss_gt"])
    loss = R.gaze_angular_loss(pred, gt)
    loss.backward()
    np.testing.assert_allclose(loss.item(), g["loss"], rtol=1e-6)
    np.testing.assert_allclose(pred.grad.numpy(), g["loss_dpred"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(g["ka_loss"], 11.706101, rtol=1e-6)
    np.testing.assert_allclose(g["ka_dpred"], [[-0.07152022, -28.50628471], [-24.10472298, 15.48111153]], rtol=1e-5)
    np.testing.assert_allclose(R.angular_error_numpy(g["loss_pred"].astype(np.float64),
                                                     g["loss_gt"].astype(np.float64))[[0, 1] + list(range(3, 32))],
                               g["ang_err_np"][[0, 1] + list(range(3, 32))], rtol=1e-9, atol=1e-9)


def test_pair_index_bit_exact(golden_dir):
    with open(os.path.join(golden_dir, "pair_index.json")) as f:
        cases = json.load(f)
    n = 0
    for key, c in cases.items():
        if key == "shared_stream":
            rng = R.MT19937(c["seed"])
            assert [list(t) for t in R.build_pair_index(c["train_rows"], "novel_train", rng)] == c["train"]
            # the test set was built from file f1 only -> file index 0 in ITS list
            assert [list(t) for t in R.build_pair_index(c["test_rows"], "novel_test", rng)] == c["test"]
            continue
        got = R.build_pair_index(c["rows"], c["tag"], R.MT19937(c["seed"]))
        assert [list(t) for t in got] == c["tuples"], key
        n += len(got)
    assert n > 1000
    a = cases["a|0|all"]["tuples"]
    assert len(a) == 76 and a[:3] == [[0, 0, 13], [0, 1, 14], [0, 2, 1]] and a[-1] == [1, 39, 36]


def test_mt19937_matches_cpython():
    import random
    for seed in (0, 1, 42, 2**40 + 17):
        random.seed(seed)
        rng = R.MT19937(seed)
        assert [random.getrandbits(32) for _ in range(1500)] == [rng.u32() for _ in range(1500)]


def _torch_sd(depth, seed=0, num_iter=3):
    return {k: torch.from_numpy(np.array(v)) for k, v in synth.make_state_dict(depth, seed, num_iter, perturb_bn=True).items()}


def _data(batch, hw, seed=1234):
    inp = synth.make_inputs(batch, 2, seed, hw)
    img, hp, gt = (torch.from_numpy(inp[k]) for k in ("img", "head_pose", "gt_gaze"))
    return {"img_0": img[:, 0].contiguous(), "img_1": img[:, 1].contiguous(),
            "rot_0": R.rotation_matrix_2d(hp[:, 0]), "rot_1": R.rotation_matrix_2d(hp[:, 1]),
            "gt_gaze": gt[:, 0].contiguous(), "gt_gaze_1": gt[:, 1].contiguous()}


def _check_outputs(data, g, prefix, rtol, num_iter=3):
    for k in ("img_feat_0", "img_feat_1", "initial_rot_feat_0", "initial_rot_feat_1", "pred_gaze"):
        ref = g[f"{prefix}.{k}"]
        np.testing.assert_allclose(data[k].detach().numpy(), ref, rtol=rtol, atol=rtol * np.abs(ref).max())
    for i in range(num_iter):
        for k in ("feat_0", "feat_1", "pred_gaze_0", "pred_gaze_1"):
            ref = g[f"{prefix}.iter_{i}.{k}"]
            np.testing.assert_allclose(data[f"iter_{i}"][k].detach().numpy(), ref, rtol=rtol,
                                       atol=rtol * np.abs(ref).max())


@pytest.mark.parametrize("depth,batch,hw", [(18, 2, 224), (50, 2, 224), (18, 3, 64), (50, 3, 64)])
def test_model_forward_backward_vs_reference(golden_dir, depth, batch, hw):
    g = _load(golden_dir, f"model_r{depth}_b{batch}_hw{hw}.npz")
    # eval
    sd = _torch_sd(depth)
    with torch.no_grad():
        data = R.model_forward(sd, _data(batch, hw), depth, 3, training=False)
    _check_outputs(data, g, "eval", 1e-6)
    # train: forward + loss + backward + running stats
    sd = _torch_sd(depth)
    leaves = {k: v.requires_grad_(True) for k, v in sd.items()
              if v.dtype == torch.float32 and "running" not in k}
    data = _data(batch, hw)
    data["img_0"].requires_grad_(True)
    data = R.model_forward(sd, data, depth, 3, training=True)
    loss = R.iteration_loss(data)
    loss.backward()
    _check_outputs(data, g, "train", 1e-6)
    np.testing.assert_allclose(loss.item(), g["train.loss"], rtol=1e-6)
    for key in [k[5:] for k in g.files if k.startswith("grad._")]:
        ref = g["grad." + key]
        got = leaves[key].grad.reshape(-1)[: ref.size].numpy()
        np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max() + 1e-12)
        np.testing.assert_allclose(float(leaves[key].grad.double().norm()), g["gradnorm." + key], rtol=1e-5)
    assert leaves["_feat_extractor.0.fc.weight"].grad is None
    np.testing.assert_allclose(data["img_0"].grad[:, :, ::16, ::16].numpy(), g["grad.img_0"], rtol=1e-5,
                               atol=1e-5 * np.abs(g["grad.img_0"]).max())
    for k in [k for k in g.files if k.startswith("stat.")]:
        np.testing.assert_allclose(sd[k[5:]].detach().numpy(), g[k], rtol=1e-6, atol=1e-7)
    assert int(sd["_feat_extractor.0.bn1.num_batches_tracked"]) == 2


def decay_sample(g):
    """make_golden.py:decay_sample - 512 elements at an even stride over the whole tensor."""
    flat = g.reshape(-1)
    return flat[::max(1, flat.numel() // 512)][:512]


def test_two_iteration_model_and_decayed_last_iteration_vs_reference(golden_dir):
    """The reference FeatRotationSymm(backbone_depth=18, num_iter=2) (make_golden.py --iter): the oracle at I = 2, same
    bars as the I = 3 fixtures above, and a second train step under IterationLoss(iter_decay=0.5, additional_decay=0.25)
    (keys decay.*: the loss, every sampled gradient's leading elements and norm)."""
    depth, batch, hw, I = 18, 3, 64, 2
    g = _load(golden_dir, "model_r18_b3_hw64_it2.npz")
    assert not [k for k in g.files if "iter_2" in k or "_img_fusers.2" in k or "_gaze_estimators.2" in k]
    assert os.path.getsize(os.path.join(golden_dir, "model_r18_b3_hw64_it2.npz")) <= os.path.getsize(
        os.path.join(golden_dir, "model_r18_b3_hw64.npz"))
    sd = _torch_sd(depth, num_iter=I)
    with torch.no_grad():
        data = R.model_forward(sd, _data(batch, hw), depth, I, training=False)
    assert data["num_iter"] == I and data["pred_gaze"] is data["iter_1"]["pred_gaze_0"] and "iter_2" not in data
    _check_outputs(data, g, "eval", 1e-6, I)
    for prefix, kw in (("", {}), ("decay.", dict(iter_decay=0.5, additional_decay=0.25))):
        sd = _torch_sd(depth, num_iter=I)
        leaves = {k: v.requires_grad_(True) for k, v in sd.items() if v.dtype == torch.float32 and "running" not in k}
        data = _data(batch, hw)
        data["img_0"].requires_grad_(True)
        data = R.model_forward(sd, data, depth, I, training=True)
        loss = R.iteration_loss(data, **kw)
        loss.backward()
        if not prefix:
            _check_outputs(data, g, "train", 1e-6, I)
        np.testing.assert_allclose(loss.item(), g["train.loss" if not prefix else "decay.loss"], rtol=1e-6)
        keys = [k[len(prefix) + 5:] for k in g.files if k.startswith(prefix + "grad._")]
        assert len(keys) == 18
        for key in keys:
            ref = g[prefix + "grad." + key]
            got = (decay_sample(leaves[key].grad) if prefix else leaves[key].grad.reshape(-1)[: ref.size]).numpy()
            assert got.shape == ref.shape and (ref.any() or not prefix), key
            np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max() + 1e-12)
            np.testing.assert_allclose(float(leaves[key].grad.double().norm()), g[prefix + "gradnorm." + key], rtol=1e-5)
        ref = g[prefix + "grad.img_0"]
        np.testing.assert_allclose(data["img_0"].grad[:, :, ::16, ::16].numpy(), ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())
        if not prefix:
            for k in [k for k in g.files if k.startswith("stat.")]:
                np.testing.assert_allclose(sd[k[5:]].detach().numpy(), g[k], rtol=1e-6, atol=1e-7)
    # the two losses (0.5 L0 + L1 against L0 + 0.25 L1) differ by far more than the 1e-6 above: the second set is no copy of the first
    assert abs(float(g["decay.loss"]) - float(g["train.loss"])) > 1e-2 * float(g["train.loss"])


def iteration_loss_cases(g):
    """(index, num_iter, iter_decay, additional_decay or None) of tests/golden/iteration_loss_decay.npz."""
    return [(i, int(n), float(d), None if a < 0 else float(a)) for i, (n, d, a) in enumerate(g["cases"])]


def test_iteration_loss_with_additional_decay_vs_reference(golden_dir):
    """oracle.restatement.iteration_loss against the reference's IterationLoss(StereoL1Loss) on every row of
    iteration_loss_decay.npz: counts 1..4, iter_decay 0.5 / 1.0, additional_decay None / 0.25 / 0.0 - loss and
    d loss / d pred of every iteration, at the bars of test_loss_known_answers."""
    g = _load(golden_dir, "iteration_loss_decay.npz")
    cases = iteration_loss_cases(g)
    assert len(cases) == 24 and {(n, d, a) for _, n, d, a in cases} == {(n, d, a) for n in (1, 2, 3, 4) for d in (0.5, 1.0) for a in (None, 0.25, 0.0)}
    gt = torch.from_numpy(g["gt"])
    assert gt.shape == (2, 5, 2)
    # the generator's condition, re-checked on what it stored: no row within 1 degree of the loss's singularities
    for it in range(4):
        for side in range(2):
            ang = R.angular_error_numpy(g["pred"][it, side].astype(np.float64), g["gt"][side].astype(np.float64))
            assert ang.min() >= 1.0 and ang.max() <= 179.0
    for idx, n, d, a in cases:
        p = torch.from_numpy(g["pred"][:n].copy()).requires_grad_(True)
        data = {"num_iter": n, "gt_gaze": gt[0], "gt_gaze_1": gt[1]}
        for it in range(n):
            data[f"iter_{it}"] = {"pred_gaze_0": p[it, 0], "pred_gaze_1": p[it, 1]}
        loss = R.iteration_loss(data, iter_decay=d, rel_weight=0.01, reference_decay=1.0, additional_decay=a)
        loss.backward()
        np.testing.assert_allclose(loss.item(), g[f"loss_{idx}"], rtol=1e-6, err_msg=str((n, d, a)))
        np.testing.assert_allclose(p.grad.numpy(), g[f"dpred_{idx}"], rtol=1e-5, atol=1e-6, err_msg=str((n, d, a)))
        if a == 0.0:
            assert not p.grad[n - 1].any() and (n == 1 or p.grad[:n - 1].abs().min() > 0)
    # None, 0.25 and 0.0 are three different losses at every count (None weighs the last iteration with 1)
    by = {(n, d, a): float(g[f"loss_{i}"]) for i, n, d, a in cases}
    for n in (1, 2, 3, 4):
        assert by[(n, 0.5, None)] != by[(n, 0.5, 0.0)] and by[(n, 0.5, 0.25)] != by[(n, 0.5, 0.0)]
    assert by[(1, 0.5, 0.0)] == 0.0


def test_multiview_loss_with_additional_decay_is_the_per_pair_mean():
    """oracle.restatement.multiview_loss(additional_decay=a): the mean over pairs of iteration_loss(..., a) on each pair."""
    g = torch.Generator().manual_seed(3)
    V, B, I = 3, 4, 3
    gt = torch.rand(B, V, 2, generator=g) - 0.5
    pairs = {}
    for (i, j) in R.view_pairs(V):
        pd = {"num_iter": I}
        for it in range(I):
            pd[f"iter_{it}"] = {"pred_gaze_0": gt[:, i] + 0.1 + 0.2 * torch.rand(B, 2, generator=g),
                                "pred_gaze_1": gt[:, j] - 0.1 - 0.2 * torch.rand(B, 2, generator=g)}
        pairs[(i, j)] = pd
    for a in (None, 0.25, 0.0):
        want = 0
        for (i, j), pd in pairs.items():
            d = dict(pd)
            d["gt_gaze"], d["gt_gaze_1"] = gt[:, i], gt[:, j]
            want = want + R.iteration_loss(d, 0.5, 0.01, 1.0, a)
        got = R.multiview_loss({"pairs": pairs}, gt, 0.5, 0.01, 1.0, a)
        assert got.item() == (want / 3).item()
    assert R.multiview_loss({"pairs": pairs}, gt, additional_decay=0.0) != R.multiview_loss({"pairs": pairs}, gt)


VARIANTS = {
    "share_weights": dict(share_weights=True),
    "ignore_rotmat": dict(ignore_rotmat=True),
    "encode_rotmat": dict(encode_rotmat=True),
    "share_feature": dict(share_feature=True),
    "share_weights_encode_rotmat": dict(share_weights=True, encode_rotmat=True),
}


def _variant_sd(variant, depth=18, seed=0):
    """state_dict as torch tensors; share_weights names map to ONE tensor object (one autograd leaf)."""
    raw = synth.make_state_dict(depth, seed, 3, perturb_bn=True, variant=variant)
    cache, sd = {}, {}
    for k, v in raw.items():
        if id(v) not in cache:
            cache[id(v)] = torch.from_numpy(np.array(v))
        sd[k] = cache[id(v)]
    return sd


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_variants_vs_reference(golden_dir, name):
    """The four ablation variants (and one combination) of /root/reference/models/rot_mv.py:136-171
    against fixtures produced by the reference itself (tests/golden/make_golden.py --variants)."""
    from rot_mvgaze_amd.arch import Variant
    variant = Variant(**VARIANTS[name]).check()
    g = _load(golden_dir, f"variant_{name}_r18_b3_hw64.npz")
    sd = _variant_sd(variant)
    with torch.no_grad():
        data = R.model_forward(sd, _data(3, 64), 18, 3, training=False, variant=variant)
    _check_outputs(data, g, "eval", 1e-6)
    sd = _variant_sd(variant)
    leaves = {k: v.requires_grad_(True) for k, v in sd.items() if v.dtype == torch.float32 and "running" not in k}
    data = R.model_forward(sd, _data(3, 64), 18, 3, training=True, variant=variant)
    loss = R.iteration_loss(data)
    loss.backward()
    _check_outputs(data, g, "train", 1e-6)
    np.testing.assert_allclose(loss.item(), g["train.loss"], rtol=1e-6)
    for key in [k[5:] for k in g.files if k.startswith("grad._")]:
        ref = g["grad." + key]
        got = leaves[key].grad.reshape(-1)[: ref.size].numpy()
        np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max() + 1e-12)
        np.testing.assert_allclose(float(leaves[key].grad.double().norm()), g["gradnorm." + key], rtol=1e-5)
    for k in [k for k in g.files if k.startswith("stat.")]:
        np.testing.assert_allclose(sd[k[5:]].detach().numpy(), g[k], rtol=1e-6, atol=1e-7)


def test_invalid_variant_combinations_raise():
    from rot_mvgaze_amd.arch import Variant
    with pytest.raises(AssertionError):
        Variant(ignore_rotmat=True, encode_rotmat=True).check()
    with pytest.raises(ValueError):
        Variant(share_feature=True, share_weights=True).check()


def test_view_swap_symmetry_is_bit_exact():
    """swapping the two views swaps the outputs bit-exactly in eval mode."""
    sd = _torch_sd(18)
    with torch.no_grad():
        a = R.model_forward(sd, _data(2, 64), 18, 3, False)
        d = _data(2, 64)
        d = {"img_0": d["img_1"], "img_1": d["img_0"], "rot_0": d["rot_1"], "rot_1": d["rot_0"]}
        b = R.model_forward(sd, d, 18, 3, False)
    for i in range(3):
        assert torch.equal(a[f"iter_{i}"]["pred_gaze_0"], b[f"iter_{i}"]["pred_gaze_1"])
        assert torch.equal(a[f"iter_{i}"]["feat_1"], b[f"iter_{i}"]["feat_0"])


def test_multiview_pairs_equal_two_view_recurrence():
    """A9: every pair (i,j) of the V-view generalisation equals the two-view oracle on views i,j
    (eval mode, shared backbone features)."""
    sd = _torch_sd(18)
    inp = synth.make_inputs(2, 3, 99, 64)
    img, hp, gt = (torch.from_numpy(inp[k]) for k in ("img", "head_pose", "gt_gaze"))
    rot = R.rotation_matrix_2d(hp.reshape(-1, 2)).reshape(2, 3, 3, 3)
    with torch.no_grad():
        mv = R.multiview_forward(sd, img, rot, 18, 3, False)
        for (i, j) in R.view_pairs(3):
            two = R.model_forward(sd, {"img_0": img[:, i], "img_1": img[:, j], "rot_0": rot[:, i], "rot_1": rot[:, j]},
                                  18, 3, False)
            for it in range(3):
                for k in ("feat_0", "feat_1", "pred_gaze_0", "pred_gaze_1"):
                    assert torch.equal(mv["pairs"][(i, j)][f"iter_{it}"][k], two[f"iter_{it}"][k])
        loss = R.multiview_loss(mv, gt)
    assert loss.ndim == 0 and torch.isfinite(loss)


def test_iteration_loss_weights():
    """IterationLoss weights are exactly (0.25, 0.5, 1.0) for decay 0.5 and 3 iterations."""
    gt = torch.tensor([[0.1, 0.2], [0.0, -0.1]])
    preds = [torch.tensor([[0.2, 0.1], [0.1, 0.0]]) * (k + 1) for k in range(3)]
    data = {"num_iter": 3, "gt_gaze": gt, "gt_gaze_1": gt}
    for i in range(3):
        data[f"iter_{i}"] = {"pred_gaze_0": preds[i], "pred_gaze_1": preds[i]}
    Ls = [R.stereo_loss(preds[i], preds[i], gt, gt) for i in range(3)]
    np.testing.assert_allclose(R.iteration_loss(data).item(), (0.25 * Ls[0] + 0.5 * Ls[1] + Ls[2]).item(), rtol=1e-6)


def _erase_inputs():
    return torch.from_numpy(synth.normal(10 * 3 * 40 * 56, 77, "erase").reshape(10, 3, 40, 56).astype(np.float32))


def test_multi_erase_draws_match_reference(golden_dir):
    """rot_mvgaze_amd.augment.RandomMultiErasing.draw replays the reference's RNG calls
    (utils/augment.py:38-45): seeded alike, the same images get the same keep-masks.  The masks are
    applied here with F.interpolate (the reference's own upsampling) - the HIP kernel is checked
    against the same fixture in tests/test_kernels_gpu.py."""
    import random
    import torch.nn.functional as F
    from rot_mvgaze_amd.augment import RandomMultiErasing
    g = _load(golden_dir, "multi_erase.npz")
    random.seed(7)
    np.random.seed(7)
    torch.manual_seed(7)
    aug = RandomMultiErasing(p=0.5, proportion=[0.5, 0.6], dot_size=[0.05, 0.3])
    imgs = _erase_inputs()
    # the reference draws image by image, interleaving the three generators: draw() keeps that order
    draws = aug.draw(10)
    out = imgs.clone()
    for i, (gs, m) in enumerate(draws):
        if gs:
            out[i] *= F.interpolate(m[None, None], (40, 56)).squeeze()
    assert np.array_equal(out.numpy(), g["out"])


RESIZE_CASES = [(2, 37, 41, 24), (1, 100, 90, 64), (1, 50, 60, 96), (1, 96, 96, 48), (1, 64, 64, 64)]   # n, h, w, size
IMAGE_MEAN, IMAGE_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)                                      # main.py:38-39


def test_resize_restatement_matches_aten_fixture(golden_dir):
    """oracle.restatement.preprocess_u8 (ToTensor -> Resize(antialias=True) -> Normalize, main.py:50-55)
    against vectors produced by the ATen op torchvision's tensor Resize calls (make_golden.py --resize;
    torchvision itself is not installed: pinned to torch.nn.functional.interpolate(antialias=True)).
    Tolerance 2e-6 absolute on the normalised values: float32 rounding order of the two passes."""
    g = _load(golden_dir, "resize_aa.npz")
    for idx, (n, h, w, size) in enumerate(RESIZE_CASES):
        u8 = g[f"u8_{idx}"]
        assert u8.shape == (n, h, w, 3)
        y = R.preprocess_u8(u8, size, IMAGE_MEAN, IMAGE_STD)
        np.testing.assert_allclose(y, g[f"y_{idx}"], rtol=0, atol=2e-6)
    # BGR input: swapping before or after the (per-channel) resize is the same thing
    u8 = g["u8_1"]
    a = R.preprocess_u8(u8, 64, IMAGE_MEAN, IMAGE_STD, swap_rb=True)
    b = R.preprocess_u8(np.ascontiguousarray(u8[..., ::-1]), 64, IMAGE_MEAN, IMAGE_STD)
    assert np.array_equal(a, b)


def test_vector_to_pitchyaw_matches_reference(golden_dir):
    """rot_mvgaze_amd.geometry.vector_to_pitchyaw (utils/math.py:62-94; imported by trainer.py:26, unused
    on the path) against the reference's own outputs, numpy (float64) and torch (float32) branches."""
    from rot_mvgaze_amd.geometry import vector_to_pitchyaw
    g = _load(golden_dir, "vector_to_pitchyaw.npz")
    np.testing.assert_allclose(vector_to_pitchyaw(g["v"].astype(np.float64)), g["py_numpy"], rtol=0, atol=1e-12)
    got = vector_to_pitchyaw(torch.from_numpy(g["v"]))
    assert got.dtype == torch.float32 and got.shape == (32, 2)
    np.testing.assert_allclose(got.numpy(), g["py_torch"], rtol=0, atol=1e-6)
    with pytest.raises(ValueError):
        vector_to_pitchyaw([[0.0, 0.0, 1.0]])


def test_conditioned_recipe_is_well_conditioned():
    """synth.make_state_dict(conditioned=True) on the CPU oracle ALONE (no kernel in the comparison): ResNet-50 with
    bf16 storage rounding (restatement.bf16_round), input perturbed by 1e-5 relative - i.e. a few flipped bf16
    roundings, which is exactly how two correct bf16 implementations differ.  The random-init recipe moves the
    predictions by > 5e-2 of their maximum (measured 1.1e-1), the conditioned one by < 1.5e-2 (measured 2-6e-3): half
    of tests/test_bf16_gpu.py's BF16_PRED_TOL = 3e-2, which that test then asserts on ResNet-50 end to end."""
    torch.set_num_threads(min(8, torch.get_num_threads()))
    depth, B, V, hw = 50, 8, 2, 128
    inp = synth.make_inputs(B, V, 5, hw)
    img, hp = torch.from_numpy(inp["img"]), torch.from_numpy(inp["head_pose"])
    rot = R.rotation_matrix_2d(hp.reshape(-1, 2)).reshape(B, V, 3, 3)

    def moved(conditioned):
        sdn = synth.make_state_dict(depth, 0, 3, perturb_bn=True, conditioned=conditioned)
        preds = []
        for x in (img, img * (1 + 1e-5)):
            sd = {k: torch.from_numpy(np.array(v)) for k, v in sdn.items()}
            with torch.no_grad():
                o = R.multiview_forward(sd, x, rot, depth, 3, True, None, R.bf16_round)
            preds.append(torch.cat([o["pairs"][(0, 1)][f"iter_{i}"][k] for i in range(3) for k in ("pred_gaze_0", "pred_gaze_1")]))
        return float((preds[1] - preds[0]).abs().max() / preds[0].abs().max())

    assert moved(True) < 1.5e-2
    assert moved(False) > 5e-2
