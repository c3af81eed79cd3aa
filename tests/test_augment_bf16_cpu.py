"""TrainAugment's bf16 destinations (mvg_augment_u8hwc_bf16), the host side: the C ABI row, the outputs TrainAugment.apply
names and refuses without a GPU, and the NumPy restatement of the two bf16 stem operands (tests/augment_bf16_ref.py)
against its definition, element by element."""
import numpy as np
import pytest
import torch

import augment_bf16_ref as W
import cabi_header as hdr
import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd.augment import TrainAugment


def test_header_binding_and_library_agree():
    import __graft_entry__ as ge
    from rot_mvgaze_amd import _lib
    name = "mvg_augment_u8hwc_bf16"
    assert hdr.functions[name][0] == "int" and hdr.arity(name) == 19
    params = hdr.functions[name][1]
    assert [p for _, p in params[:5]] == ["src", "recs", "recs_host", "dst_nhwc8", "dst_rw"]
    assert [t for t, _ in params[3:5]] == ["uint16_t*", "uint16_t*"]
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 19
    ge.build()
    assert hasattr(_lib.lib(), name)
    assert hdr.constants["MVG_ABI_VERSION"] == _lib.ABI_VERSION            # additive: the version is test_cabi_cpu's pin


@pytest.mark.parametrize("out", ["rw_bf16", "nhwc8_bf16"])
def test_bf16_outputs_have_no_cpu_fallback(out):
    aug = TrainAugment()
    u8 = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        aug.apply(u8, aug.draw(1, 8, 8), out=out)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        aug(u8, out=out)


def test_unknown_out_and_mixed_destinations_raise_value_error():
    aug = TrainAugment()
    u8 = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="out must be"):                   # before the device check
        aug.apply(u8, aug.draw(1, 8, 8), out="bogus")
    d4 = torch.empty(1, 8, 8, 4)
    d8 = torch.empty(1, 8, 8, 8, dtype=torch.bfloat16)
    rw = torch.empty(1, 8, 2, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="a launch each"):
        aug.launch(u8, aug.draw(1, 8, 8), None, d4, False, dst_nhwc8=d8)
    with pytest.raises(ValueError, match="a launch each"):
        aug.launch(u8, aug.draw(1, 8, 8), torch.empty(1, 8, 8, 3, dtype=torch.uint8), None, dst_rw=rw)


@pytest.mark.parametrize("n,h,w", [(2, 3, 4), (1, 2, 12)])
def test_window_helper_against_its_definition(n, h, w):
    """xw[i, y, m, 4j + c] = img[i, y, 4m - 4 + j, c] for 0 <= 4m - 4 + j < w and c < 3, else 0 - in plain loops."""
    rng = np.random.RandomState(n * 100 + w)
    img = rng.randint(1, 30000, (n, h, w, 3)).astype(np.int16)             # no zero: a value is never mistaken for padding
    xw, x8 = W.row_windows(img), W.nhwc8(img)
    assert xw.shape == (n, h, w // 4, 64) and xw.dtype == img.dtype
    assert x8.shape == (n, h, w, 8) and x8.dtype == img.dtype
    for i in range(n):
        for y in range(h):
            for m in range(w // 4):
                for j in range(16):
                    for c in range(4):
                        col = 4 * m - 4 + j
                        want = img[i, y, col, c] if (0 <= col < w and c < 3) else 0
                        assert xw[i, y, m, 4 * j + c] == want, (i, y, m, j, c)
            for x in range(w):
                for c in range(8):
                    assert x8[i, y, x, c] == (img[i, y, x, c] if c < 3 else 0), (i, y, x, c)


def test_every_pixel_lands_in_up_to_four_windows():
    """A pixel's values appear once in every window whose 16 columns hold it: four, fewer where the row's windows stop."""
    img = np.arange(1, 1 + 2 * 20 * 3, dtype=np.int16).reshape(1, 2, 20, 3)
    xw = W.row_windows(img)
    for x in range(20):
        windows = [m for m in range(5) if 0 <= x - (4 * m - 4) < 16]
        assert (xw == img[0, 1, x, 0]).sum() == len(windows)
        assert len(windows) == (4 if 8 <= x < 16 else 3 if 4 <= x else 2)
