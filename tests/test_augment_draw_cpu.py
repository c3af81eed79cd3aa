"""TrainAugment(draws="device"), the host side (no GPU): Philox4x32-10 known answers and the distributions of the NumPy
restatement (tests/augment_draw_ref.py) that the GPU tests compare the device against bit for bit, the C ABI row of
mvg_augment_draw and its settings struct, the checks it makes before any launch, and the Python surface."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import augment_draw_ref as R
import cabi_header as hdr
import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd.augment import DRAW_CFG_DTYPE, REC_DTYPE, RandomMultiErasing, TrainAugment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, N, H, W = 20261020, 6000, 224, 224                # the seed is chosen so that the restatement meets the bounds below


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from rot_mvgaze_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def drawn():
    return R.draw(N, H, W, SEED, 0, **R.RECIPE)


# ---------------------------------------------------------------- the generator
@pytest.mark.parametrize("counter,key,want", [
    ([0, 0, 0, 0], (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xFFFFFFFF] * 4, (0xFFFFFFFF, 0xFFFFFFFF), "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox_known_answers(counter, key, want):
    got = R.philox4x32_10(np.array(counter, np.uint32), key)
    assert " ".join(f"{int(v):08x}" for v in got) == want
    many = R.philox4x32_10(np.array([counter, [1, 2, 3, 4]], np.uint32), key)          # and as one row of a batch
    assert " ".join(f"{int(v):08x}" for v in many[0]) == want


def test_uniform_is_exact_and_below_one():
    u = R.u01(np.array([0, 255, 256, 0xFFFFFFFF], np.uint32))
    assert u.dtype == np.float32 and u.tolist() == [0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24]


# ---------------------------------------------------------------- the distributions of the restatement (reference recipe)
def test_orders_and_factors(drawn):
    recs = drawn[0]
    assert recs.dtype == R.REC == REC_DTYPE and recs.shape == (N,)
    assert (np.sort(recs["order"], 1) == [0, 1, 2]).all()
    sd = np.sqrt(N * (1 / 6) * (5 / 6))
    for perm in R.PERMS:
        count = int((recs["order"] == perm).all(1).sum())
        assert abs(count - N / 6) <= 5 * sd, (perm, count)
    for op, (lo, hi) in enumerate([(0.0, 2.0), (0.9, 1.1), (0.9, 1.1)]):
        f = recs["factor"][:, op]
        assert (f >= np.float32(lo)).all() and (f < np.float32(hi)).all(), op       # the range's float32 end points
        assert abs(float(f.astype(np.float64).mean()) - (lo + hi) / 2) <= 5 * (hi - lo) / np.sqrt(12 * N), op


def test_affine_map(drawn):
    recs, extras = drawn[0], drawn[3]
    for t in (extras["tx"], extras["ty"]):
        assert set(t.tolist()) == {-2, -1, 0, 1, 2}
    s = extras["scale"]
    assert s.dtype == np.float32 and (s >= np.float32(0.99)).all() and (s <= np.float32(1.01)).all()
    assert (recs["a0"] == recs["a4"]).all() and (recs["a0"] == 1.0 / s.astype(np.float64)).all()
    assert (recs["cx"] == recs["a0"] * (-112.0 - extras["tx"]) + 112.0).all()
    assert (recs["cy"] == recs["a4"] * (-112.0 - extras["ty"]) + 112.0).all()


def test_erase(drawn):
    _, masks, grid, extras = drawn
    p = R.RECIPE["erase"]["p"]
    assert R.gmax_of(R.RECIPE["erase"]) == 20 and masks.shape == (N, 400) and masks.dtype == np.float32 and grid.dtype == np.int32
    erased = grid > 0
    assert (erased == extras["applied"]).all()
    assert abs(erased.mean() - p) <= 5 * np.sqrt(p * (1 - p) / N)
    g = grid[erased].astype(np.int64)
    assert g.min() >= 3 and g.max() <= 20 and len(set(g.tolist())) >= 15
    assert set(np.unique(masks).tolist()) == {0.0, 1.0}
    assert not masks[~erased].any()                                     # an image left alone: an all-zero slot
    inside = np.arange(400)[None, :] < (g ** 2)[:, None]
    assert not masks[erased][~inside].any()                             # cells past g*g are zero
    # kept fraction over the cells of the erased images against its expectation, the cell-weighted mean of 1 - prop
    cells = int((g ** 2).sum())
    q = 1.0 - float((extras["prop"][erased] * g ** 2).sum() / cells)
    kept = float(masks[erased].sum()) / cells
    assert 0.4 <= q <= 0.5 and abs(kept - q) <= 5 * np.sqrt(q * (1 - q) / cells), (kept, q)


def test_seed_and_counter_move_the_draws(drawn):
    recs = drawn[0]
    small = dict(R.RECIPE)
    a = R.draw(16, H, W, SEED, 0, **small)
    assert a[0].tobytes() == recs[:16].tobytes()                        # image i does not depend on n
    for seed, counter in ((SEED + 1, 0), (SEED, 1), (SEED + (1 << 32), 0), (SEED, 1 << 32)):
        b = R.draw(16, H, W, seed, counter, **small)
        assert b[0].tobytes() != a[0].tobytes() and b[1].tobytes() != a[1].tobytes(), (seed, counter)
    # the word assignment is fixed: switching the erase off leaves the records where they are
    assert R.draw(16, H, W, SEED, 0, **dict(small, erase=None))[0].tobytes() == a[0].tobytes()
    # disabled ops: exactly the identity
    r = R.draw(16, 17, 23, SEED, 3, brightness=0.0, contrast=0.0, saturation=0.0, scale=None, translate=None)[0]
    assert (r["factor"] == 1.0).all() and (r["a0"] == 1.0).all() and (r["cx"] == 0.0).all() and (r["cy"] == 0.0).all()


# ---------------------------------------------------------------- the C ABI
def _cfg_struct():
    """mvg_augment_draw_cfg as include/rotmvgaze_augment_draw.h declares it, read by the header parser (which knows one include
    guard, rotmvgaze.h's: this header's preprocessor lines are dropped first)."""
    with open(os.path.join(ROOT, "include", "rotmvgaze_augment_draw.h")) as f:
        text = "\n".join(line for line in f.read().split("\n") if not line.lstrip().startswith("#"))
    functions, structs, constants = hdr.parse(text)
    assert not functions and not constants and list(structs) == ["mvg_augment_draw_cfg"]
    return structs["mvg_augment_draw_cfg"]


def test_abi_row(built_lib):
    from rot_mvgaze_amd import _lib
    assert hdr.functions["mvg_augment_draw"][0] == "int"
    assert hdr.parameter_names("mvg_augment_draw") == ["recs", "masks", "grid", "gmax", "n", "h", "w", "cfg", "seed", "counter_dev", "stream"]
    assert [t for t, _ in hdr.functions["mvg_augment_draw"][1]] == ["mvg_augment_rec*", "float*", "int32_t*", "int", "int", "int", "int",
                                                                   "void*", "uint64_t", "uint64_t*", "void*"]
    assert "mvg_augment_draw" in _lib.SIGNATURES and hasattr(built_lib, "mvg_augment_draw")
    res, args = _lib.SIGNATURES["mvg_augment_draw"]
    assert res is C.c_int and len(args) == hdr.arity("mvg_augment_draw") == 11 and args[8] is C.c_uint64
    assert hdr.constants["MVG_ABI_VERSION"] == _lib.ABI_VERSION == built_lib.mvg_abi_version() == 13          # additive


def test_cfg_struct_is_the_dtype_the_host_packs():
    scalars = {"float": (np.float32, C.c_float), "double": (np.float64, C.c_double), "int32_t": (np.int32, C.c_int32)}
    fields = _cfg_struct()
    assert [n for n, _, _ in fields] == list(DRAW_CFG_DTYPE.names)
    offset = align = 0
    for name, base, length in fields:
        np_t, c_t = scalars[base]
        sub, at = DRAW_CFG_DTYPE.fields[name][:2]
        assert sub.base == np.dtype(np_t) and sub.shape == ((length,) if length else ()), name
        offset = -(-offset // C.alignment(c_t)) * C.alignment(c_t)           # natural C alignment
        assert at == offset, f"{name}: packed at {at}, C puts it at {offset}"
        offset += C.sizeof(c_t) * (length or 1)
        align = max(align, C.alignment(c_t))
    assert DRAW_CFG_DTYPE.itemsize == -(-offset // align) * align == 88
    # ... and what TrainAugment packs into it
    aug = TrainAugment(contrast=0.0, erase=RandomMultiErasing([0.5, 0.6], 0.25, [0.05, 0.3]), draws="device", seed=1)
    cfg = aug._draw_cfg(224, 200)
    assert cfg.dtype == DRAW_CFG_DTYPE and cfg.shape == (1,) and aug._draw_cfg(224, 200) is cfg and aug._draw_cfg(200, 224) is not cfg
    assert cfg["factor_lo"][0].tolist() == [0.0, 1.0, np.float32(0.9)] and cfg["factor_hi"][0].tolist() == [2.0, 1.0, np.float32(1.1)]
    assert cfg["max_dx"][0] == np.float32(0.01 * 200) and cfg["max_dy"][0] == np.float32(0.01 * 224)
    assert (cfg["scale_lo"][0], cfg["scale_hi"][0]) == (np.float32(0.99), np.float32(1.01))
    assert (cfg["erase"][0], cfg["p"][0], cfg["prop_lo"][0], cfg["prop_hi"][0], cfg["dot_lo"][0], cfg["dot_hi"][0]) == (1, 0.25, 0.5, 0.6, 0.05, 0.3)
    off = TrainAugment(scale=None, translate=None, draws="device", seed=1)._draw_cfg(8, 8)
    assert (off["max_dx"][0], off["max_dy"][0], off["scale_lo"][0], off["scale_hi"][0], off["erase"][0]) == (0.0, 0.0, 1.0, 1.0, 0)


def test_host_checks_reject_before_any_launch(built_lib):
    """Every call here stops at a host check (status 2, a message through mvg_last_error): the pointers are host addresses
    that stand for device buffers and are never followed."""
    buf = (C.c_uint64 * 8)()
    fake = C.addressof(buf)
    erase = TrainAugment(erase=RandomMultiErasing([0.5, 0.6], 0.5, [0.05, 0.3]), draws="device", seed=1)._draw_cfg(8, 8)
    plain = TrainAugment(draws="device", seed=1)._draw_cfg(8, 8)
    fine = np.zeros(1, DRAW_CFG_DTYPE)
    fine[0] = erase[0]
    fine["dot_lo"] = 0.01                                             # (int)(1.0 / 0.01) = 100 cells a side

    def call(recs, masks, grid, gmax, n, cfg, counter):
        return built_lib.mvg_augment_draw(recs, masks, grid, gmax, n, 8, 8, C.c_void_p(cfg.ctypes.data), 1, counter, None)

    cases = [("records", (None, None, None, 0, 1, plain, fake)),
             ("counter", (fake, None, None, 0, 1, plain, None)),
             ("bad sizes", (fake, None, None, 0, 0, plain, fake)),
             ("bad sizes", (fake, None, None, 0, -3, plain, fake)),
             ("come together", (fake, fake, None, 20, 1, erase, fake)),
             ("come together", (fake, None, fake, 20, 1, erase, fake)),
             ("masks are missing", (fake, None, None, 0, 1, erase, fake)),
             ("gmax is 19", (fake, fake, fake, 19, 1, erase, fake)),
             ("gmax is 0", (fake, fake, fake, 0, 1, erase, fake)),
             ("gmax is 20 without masks", (fake, None, None, 20, 1, plain, fake)),
             ("not served", (fake, fake, fake, 100, 1, fine, fake))]
    for want, args in cases:
        assert call(*args) == 2, want
        assert want in built_lib.mvg_last_error().decode(), (want, built_lib.mvg_last_error())


# ---------------------------------------------------------------- the Python surface
def test_python_surface():
    assert TrainAugment(draws="device", seed=1).capturable is True
    assert TrainAugment().capturable is False and TrainAugment(draws="host").capturable is False
    for kw in ({"draws": "gpu"}, {"draws": "device"}, {"draws": "device", "seed": 1 << 64}, {"draws": "device", "seed": -1},
               {"draws": "device", "seed": 1.5}, {"draws": "device", "seed": True}):
        with pytest.raises(ValueError):
            TrainAugment(**kw)
    TrainAugment(draws="device", seed=(1 << 64) - 1)
    for erase in (RandomMultiErasing([0.5, 0.6], 0.5, [0.01, 0.3]),          # a grid of 100 cells a side
                  RandomMultiErasing([0.5, 0.6], 1.5, [0.05, 0.3]), RandomMultiErasing([0.5, 0.6], 0.5, [0.0, 0.3]),
                  RandomMultiErasing([0.5, 0.6], 0.5, [0.3, 0.05]), RandomMultiErasing([0.5, 0.6], 0.5, [0.05, 1.3])):
        with pytest.raises(ValueError):
            TrainAugment(erase=erase, draws="device", seed=1)
        TrainAugment(erase=erase)                                           # host draws take what the reference takes
    TrainAugment(erase=RandomMultiErasing([0.5, 0.6], 0.5, [1 / 64, 0.3]), draws="device", seed=1)
    aug = TrainAugment(draws="device", seed=7)
    for device in ("cpu", torch.device("cpu")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            aug.draw_device(2, 8, 8, device)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        aug(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="draws='device'"):
        TrainAugment().draw_device(2, 8, 8, "cuda:0")
    # the state travels without a device: the counter a later first launch starts from
    assert aug.state_dict() == {"seed": 7, "counter": 0}
    aug.load_state_dict({"seed": 9, "counter": (1 << 64) - 2})
    assert aug.state_dict() == {"seed": 9, "counter": (1 << 64) - 2}

