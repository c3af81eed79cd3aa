"""ColorJitter / RandomAffine on the GPU, the host side: the NumPy restatement (tests/augment_ref.py) against the Pillow
fixture and against Pillow itself, TrainAugment's draws, the settings it refuses, and the C ABI row."""
import os

import numpy as np
import pytest
import torch

import augment_ref as R
import cabi_header as hdr
import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd.augment import REC_DTYPE, RandomMultiErasing, TrainAugment, inverse_affine



def load_cases(golden_dir):
    g = np.load(os.path.join(golden_dir, "color_affine.npz"))
    n = len(g["swap"])
    return [(g[f"in_{k:02d}"], g["factors"][k], g["order"][k], g["matrix"][k], int(g["swap"][k]), g[f"out_{k:02d}"]) for k in range(n)]


def test_fixture_covers_what_it_must(golden_dir):
    cases = load_cases(golden_dir)
    assert 25 <= len(cases) <= 40
    assert {tuple(int(o) for o in c[2]) for c in cases} == {(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)}
    assert {int(c[4]) for c in cases} == {0, 1}
    fs = np.concatenate([c[1] for c in cases])
    for f in (0.0, 1.0, 2.0, 0.9, 1.1):
        assert (fs == f).any(), f
    assert any(c[3][0] < 1.0 for c in cases) and any(c[3][0] > 1.0 for c in cases)          # scale above and below 1
    shapes = {c[0].shape[:2] for c in cases}
    assert (1, 2) in shapes and all(h <= 40 and w <= 56 for h, w in shapes)
    assert any(h != w and h % 2 and w % 2 and (h * w) % 64 for h, w in shapes)
    assert any((c[0] == c[0].flat[0]).all() and c[0].size > 6 for c in cases)               # a constant image
    sides = set()
    for img, _, _, m, _, _ in cases:                  # fill on each of the four sides
        h, w = img.shape[:2]
        xt, yt = R.axis_table(w, m[0], m[1]), R.axis_table(h, m[2], m[3])
        sides |= {s for s, hit in (("left", xt[0] < 0), ("right", xt[-1] < 0), ("top", yt[0] < 0), ("bottom", yt[-1] < 0)) if hit}
    assert sides == {"left", "right", "top", "bottom"}


def test_restatement_equals_fixture(golden_dir):
    for k, (img, factors, order, matrix, swap, want) in enumerate(load_cases(golden_dir)):
        assert np.array_equal(R.augment(img, factors, order, matrix, swap), want), k


def test_half_mean_rounds_up():
    img = np.array([[[10, 10, 10], [11, 11, 11]]], np.uint8)
    assert R.contrast_mean(img) == 11
    assert np.array_equal(R.enhance(img, R.CONTRAST, 0.0), np.full_like(img, 11))


def test_restatement_equals_pillow():
    pytest.importorskip("PIL")
    from PIL import Image, ImageEnhance
    enh = {R.BRIGHTNESS: ImageEnhance.Brightness, R.CONTRAST: ImageEnhance.Contrast, R.SATURATION: ImageEnhance.Color}
    rng = np.random.RandomState(5)
    for k in range(24):
        h, w = [(1, 1), (7, 13), (40, 56), (64, 64), (100, 160), (224, 224)][k % 6]
        img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        factors = [(0.0, 1.0, 2.0)[(k + j) % 3] if k < 6 else 2.0 * rng.rand() for j in range(3)]
        order = rng.permutation(3)
        matrix = R.affine_matrix(h, w, 0.8 + 0.45 * rng.rand(), int(rng.randint(-w // 5 - 1, w // 5 + 2)), int(rng.randint(-h // 5 - 1, h // 5 + 2)))
        pil = Image.fromarray(img, "RGB")
        for op in order:
            pil = enh[int(op)](pil).enhance(float(factors[int(op)]))
        pil = pil.transform((w, h), Image.AFFINE, [matrix[0], 0.0, matrix[1], 0.0, matrix[2], matrix[3]], Image.NEAREST)
        assert np.array_equal(R.augment(img, factors, order, matrix), np.asarray(pil)), k


def test_draw_is_deterministic_and_in_range():
    aug = TrainAugment()
    torch.manual_seed(11)
    a = aug.draw(64, 224, 200)
    torch.manual_seed(11)
    b = aug.draw(64, 224, 200)
    assert a.recs.dtype == REC_DTYPE and a.recs.tobytes() == b.recs.tobytes() and a.erase is None
    torch.manual_seed(12)
    assert aug.draw(64, 224, 200).recs.tobytes() != a.recs.tobytes()
    h, w = 224, 200
    seen = set()
    for r in a.recs:
        assert sorted(r["order"].tolist()) == [0, 1, 2]
        seen.add(tuple(r["order"].tolist()))
        assert 0.0 <= r["factor"][0] <= 2.0 and 0.9 <= r["factor"][1] <= 1.1 and 0.9 <= r["factor"][2] <= 1.1
        assert r["a0"] == r["a4"]
        scale = 1.0 / r["a0"]
        assert 0.99 - 1e-12 <= scale <= 1.01 + 1e-12
        # c = a*(-c0 - t) + c0  ->  t = (c0 - c)/a - c0: an integer within +-round(0.01 * side)
        tx, ty = (w * 0.5 - r["cx"]) / r["a0"] - w * 0.5, (h * 0.5 - r["cy"]) / r["a4"] - h * 0.5
        assert abs(tx - round(tx)) < 1e-9 and abs(ty - round(ty)) < 1e-9
        assert abs(round(tx)) <= round(0.01 * w) and abs(round(ty)) <= round(0.01 * h)
    assert len(seen) == 6
    assert inverse_affine(40, 56, 1.25, 3, -2) == R.affine_matrix(40, 56, 1.25, 3, -2)


def test_draw_order_of_calls():
    """The documented order, replayed by hand: randperm(4), three factor draws, the angle, tx, ty, the scale, the erase."""
    import random
    aug = TrainAugment(erase=RandomMultiErasing(p=0.5, proportion=[0.5, 0.6], dot_size=[0.05, 0.3]))
    for seed in (1, 2):
        torch.manual_seed(seed), random.seed(seed), np.random.seed(seed)
        got = aug.draw(3, 224, 224)
        torch.manual_seed(seed), random.seed(seed), np.random.seed(seed)
        for i in range(3):
            order = [op for op in torch.randperm(4).tolist() if op != 3]
            fb = float(torch.empty(1).uniform_(0.0, 2.0))
            fc = float(torch.empty(1).uniform_(0.9, 1.1))
            fs = float(torch.empty(1).uniform_(0.9, 1.1))
            torch.empty(1).uniform_(0.0, 0.0)
            tx = int(round(torch.empty(1).uniform_(-2.24, 2.24).item()))
            ty = int(round(torch.empty(1).uniform_(-2.24, 2.24).item()))
            scale = float(torch.empty(1).uniform_(0.99, 1.01).item())
            (g, mask), = aug.erase.draw(1)
            r = got.recs[i]
            assert r["order"].tolist() == order
            assert r["factor"].tolist() == [np.float32(fb), np.float32(fc), np.float32(fs)]
            assert (r["a0"], r["cx"], r["a4"], r["cy"]) == R.affine_matrix(224, 224, scale, tx, ty)
            assert got.erase[i][0] == g and torch.equal(got.erase[i][1], mask)
    # an op whose range is [1, 1] draws nothing and leaves the factor at 1
    torch.manual_seed(3)
    r = TrainAugment(contrast=0.0, scale=None, translate=None).draw(2, 8, 8).recs
    assert (r["factor"][:, 1] == 1.0).all() and (r["a0"] == 1.0).all() and (r["cx"] == 0.0).all() and (r["cy"] == 0.0).all()


def test_unsupported_settings_raise():
    for kw in ({"hue": 0.1}, {"degrees": 5}, {"degrees": (-3, 3)}, {"shear": 2.0}, {"shear": (0, 0, 1, 1)}):
        with pytest.raises(NotImplementedError):
            TrainAugment(**kw)
    TrainAugment(hue=0.0, degrees=0, shear=None)
    with pytest.raises(ValueError):
        TrainAugment(brightness=-0.1)
    with pytest.raises(ValueError):
        TrainAugment(scale=(0.0, 1.0))
    with pytest.raises(ValueError):
        TrainAugment(translate=(0.1, 1.5))
    aug = TrainAugment()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        aug(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        aug.apply(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), aug.draw(1, 8, 8), out="chw")


def test_graphed_step_refuses_an_augmenting_model():
    from rot_mvgaze_amd.graph import GraphedStep
    from rot_mvgaze_amd.model import FeatRotationSymm
    m = FeatRotationSymm(18, 1)
    assert m.input_augment is None
    m.input_augment = TrainAugment()
    with pytest.raises(RuntimeError, match="cannot be captured"):
        GraphedStep(m, lambda: None)


def test_header_row_and_abi():
    assert hdr.functions["mvg_augment_u8hwc"][0] == "int" and hdr.arity("mvg_augment_u8hwc") == 19
    # the record the header declares is the record the host packs: 3 floats, 3 int32, 4 doubles at 24..56
    assert hdr.structs["mvg_augment_rec"] == [("factor", "float", 3), ("order", "int32_t", 3), ("a0", "double", None),
                                              ("cx", "double", None), ("a4", "double", None), ("cy", "double", None)]
    assert REC_DTYPE.itemsize == 56 and [REC_DTYPE.fields[k][1] for k in ("factor", "order", "a0", "cx", "a4", "cy")] == [0, 12, 24, 32, 40, 48]
