"""The random part of the reference's training transform on device batches (SURVEY.md §8(f) rank 3,
main.py:41-49): RandomMultiErasing, its last step (main.py:48, utils/augment.py:10-47),
and TrainAugment - ColorJitter and RandomAffine on the raw uint8 patches, with ToTensor, Normalize and the erase in
the same launch.

By default the random draws are made on the host and replay the reference's calls in its order - per image:
``random.random()`` (apply?), ``np.random.uniform(*dot_size)``, ``np.random.uniform(*proportion)``,
``torch.rand(g, g)`` with g = int(1 / dot_size) - so a run seeded like the reference erases the
same cells.  The multiply runs in one HIP launch over the whole batch (mvg_multi_erase_nchw).

``TrainAugment(draws="device", seed=...)`` makes its draws on the device instead (mvg_augment_draw: Philox4x32-10 keyed by
the seed, counted by a launch counter in device memory): the reference's distributions, not its RNG stream; no host draw,
no host-to-device copy and no synchronisation per step, so a step on raw patches can be captured (graph.GraphedStep).
"""
from __future__ import annotations

import random
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .backbone import IMAGE_MEAN, IMAGE_STD

Tensor = torch.Tensor


class RandomMultiErasing:
    def __init__(self, proportion: Sequence[float], p: float, dot_size: Sequence[float]):
        self.proportion = proportion
        self.p = p
        self.dot_size = dot_size

    def draw(self, n: int) -> List[Tuple[int, Tensor]]:
        """The reference's per-image draws (augment.py:38-45, :16-20) for n images: [(g, keep-mask g x g)],
        g == 0 for an image that is left alone."""
        out = []
        for _ in range(n):
            if random.random() > self.p:
                out.append((0, torch.zeros(0, 0)))
                continue
            dot_size = np.random.uniform(*self.dot_size)
            proportion = np.random.uniform(*self.proportion)
            g = int(1 / dot_size)
            mask = (torch.rand(g, g) > proportion).to(torch.float32)
            out.append((g, mask))
        return out

    def apply(self, img: Tensor, draws: List[Tuple[int, Tensor]]) -> Tensor:
        """img [B,C,H,W] fp32 on the GPU, erased in place (the reference's ``img *= mask``)."""
        if not img.is_cuda:
            raise RuntimeError("RandomMultiErasing (MI355X build) works on device batches: no CPU fallback")
        assert img.dim() == 4 and img.dtype == torch.float32 and img.is_contiguous() and len(draws) == img.shape[0]
        B, C, H, W = img.shape
        gmax = max(1, max(g for g, _ in draws))
        masks = torch.zeros(B, gmax * gmax, dtype=torch.float32)
        grid = torch.zeros(B, dtype=torch.int32)
        for i, (g, m) in enumerate(draws):
            grid[i] = g
            if g:
                masks[i, : g * g] = m.reshape(-1)
        ops.multi_erase_nchw(img, masks.to(img.device), grid.to(img.device), gmax, B, C, H, W)
        return img

    def __call__(self, img: Tensor) -> Tensor:
        """[B,C,H,W] (or one image [C,H,W]) device tensor -> erased in place, one draw per image."""
        one = img.dim() == 3
        x = img.unsqueeze(0) if one else img
        self.apply(x, self.draw(x.shape[0]))
        return img


# mvg_augment_rec (include/rotmvgaze.h): one record per image, 56 bytes
REC_DTYPE = np.dtype([("factor", np.float32, 3), ("order", np.int32, 3), ("a0", np.float64), ("cx", np.float64),
                      ("a4", np.float64), ("cy", np.float64)], align=True)
assert REC_DTYPE.itemsize == 56
BRIGHTNESS, CONTRAST, SATURATION = 0, 1, 2          # op ids of a record's order


class AugmentDraws(NamedTuple):
    recs: np.ndarray                                   # [n] REC_DTYPE
    erase: Optional[List[Tuple[int, Tensor]]]          # RandomMultiErasing.draw's list, or None


# mvg_augment_draw_cfg (include/rotmvgaze_augment_draw.h): the settings of the device draws, 88 bytes
DRAW_CFG_DTYPE = np.dtype([("factor_lo", np.float32, 3), ("factor_hi", np.float32, 3), ("max_dx", np.float32), ("max_dy", np.float32),
                           ("scale_lo", np.float32), ("scale_hi", np.float32), ("erase", np.int32), ("p", np.float64),
                           ("prop_lo", np.float64), ("prop_hi", np.float64), ("dot_lo", np.float64), ("dot_hi", np.float64)], align=True)
assert DRAW_CFG_DTYPE.itemsize == 88
MAX_DRAW_GRID = 64                                     # the widest mask grid mvg_augment_draw serves


class DeviceDraws(NamedTuple):
    """What TrainAugment.draw_device queued on the current stream: the operands of the pixel launch, in device memory."""
    recs: Tensor                                       # uint8 [n * 56]: n mvg_augment_rec
    masks: Optional[Tensor]                            # fp32 [n, gmax * gmax] keep-masks (row stride g), or None: no erase
    grid: Optional[Tensor]                             # int32 [n]: g per image, 0 = not erased
    gmax: int

    def to_host(self) -> AugmentDraws:
        """The same draws as TrainAugment.draw would hand them over (synchronises: for tests and debugging)."""
        recs = self.recs.cpu().numpy().view(REC_DTYPE).copy()
        if self.masks is None:
            return AugmentDraws(recs, None)
        masks, grid = self.masks.cpu(), self.grid.cpu().tolist()
        return AugmentDraws(recs, [(g, masks[i, : g * g].reshape(g, g).clone()) if g else (0, torch.zeros(0, 0))
                                   for i, g in enumerate(grid)])


def inverse_affine(h: int, w: int, scale: float, tx: float, ty: float) -> Tuple[float, float, float, float]:
    """torchvision's _get_inverse_affine_matrix for angle 0 and no shear about the centre (w/2, h/2), in Python doubles
    and in its order of operations: (a0, c_x, a4, c_y); the off-diagonal terms are exactly zero."""
    cx, cy = w * 0.5, h * 0.5
    a0 = a4 = 1.0 / scale
    return a0, a0 * (-cx - tx) + cx, a4, a4 * (-cy - ty) + cy


def _jitter_range(name: str, value: float) -> Optional[Tuple[float, float]]:
    """ColorJitter._check_input for a scalar: [max(0, 1 - v), 1 + v], None (no draw, op left out) when that is [1, 1]."""
    if value < 0:
        raise ValueError(f"If {name} is a single number, it must be non negative.")
    lo, hi = max(0.0, 1.0 - float(value)), 1.0 + float(value)
    return None if lo == hi == 1.0 else (lo, hi)


class TrainAugment:
    """ColorJitter(brightness, contrast, saturation) -> RandomAffine(degrees=0, scale, translate) -> ToTensor ->
    Normalize -> RandomMultiErasing of main.py:41-49 on a device batch of raw uint8 [n, h, w, 3] patches, one HIP launch
    (mvg_augment_u8hwc; mvg_augment_u8hwc_bf16 stores the bf16 stem's operand instead).  The pixel arithmetic is Pillow's, bit for bit (what torchvision runs on the PIL image; pinned by
    tests/golden/color_affine.npz).  Patches keep their size: the reference's Resize(224) is the identity on the
    datasets' 224 x 224 patches, and a resize after the augmentation is not served.

    hue, rotation and shear take other Pillow code paths and raise NotImplementedError here."""

    def __init__(self, brightness: float = 1.0, contrast: float = 0.1, saturation: float = 0.1,
                 scale: Optional[Sequence[float]] = (0.99, 1.01), translate: Optional[Sequence[float]] = (0.01, 0.01),
                 erase: Optional[RandomMultiErasing] = None, hue: float = 0.0, degrees: float = 0.0, shear=None,
                 draws: str = "host", seed: Optional[int] = None):
        if hue is not None and any(float(v) != 0.0 for v in np.atleast_1d(hue)):
            raise NotImplementedError("TrainAugment: hue jitter (an HSV round trip in Pillow) is not implemented")
        if any(float(v) != 0.0 for v in np.atleast_1d(degrees)):
            raise NotImplementedError("TrainAugment: rotation (Pillow's general affine path) is not implemented: degrees must be 0")
        if shear is not None and any(float(v) != 0.0 for v in np.atleast_1d(shear)):
            raise NotImplementedError("TrainAugment: shear (Pillow's general affine path) is not implemented")
        self.ranges = [_jitter_range("brightness", brightness), _jitter_range("contrast", contrast),
                       _jitter_range("saturation", saturation)]
        if scale is not None and not (len(scale) == 2 and 0 < scale[0] <= scale[1]):
            raise ValueError("scale must be (low, high) with 0 < low <= high")
        if translate is not None and not (len(translate) == 2 and all(0.0 <= t <= 1.0 for t in translate)):
            raise ValueError("translation values should be between 0 and 1")
        self.scale, self.translate, self.erase = scale, translate, erase
        if draws not in ("host", "device"):
            raise ValueError(f"draws must be 'host' or 'device' (got {draws!r})")
        self.draws, self.seed = draws, seed
        self._gmax = 0
        self._counter: Optional[Tensor] = None         # device int64 [1]: the launch counter (created on first use, never replaced)
        self._counter_start = 0                        # ... its value until then
        self._cfgs = {}                                # (h, w) -> one DRAW_CFG_DTYPE element
        if draws == "device":
            if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
                raise ValueError(f"draws='device' needs seed = an int of at most 64 bits (got {seed!r})")
            if erase is not None:
                (dot_lo, dot_hi), p = (float(v) for v in erase.dot_size), float(erase.p)
                if len(erase.proportion) != 2 or not (0.0 <= p <= 1.0 and 0.0 < dot_lo <= dot_hi <= 1.0):
                    raise ValueError("draws='device' with an erase needs 0 <= p <= 1, 0 < dot_size[0] <= dot_size[1] <= 1 and a "
                                     "(low, high) proportion")
                self._gmax = int(1.0 / dot_lo)
                if self._gmax > MAX_DRAW_GRID:
                    raise ValueError(f"draws='device': dot_size[0] = {dot_lo} gives a mask grid of {self._gmax} cells a side "
                                     f"(at most {MAX_DRAW_GRID})")

    @property
    def capturable(self) -> bool:
        """Whether a step that applies this augment can be captured (graph.GraphedStep): the draws are device work."""
        return self.draws == "device"

    def _draw_cfg(self, h: int, w: int) -> np.ndarray:
        cfg = self._cfgs.get((h, w))
        if cfg is None:
            cfg = np.zeros(1, dtype=DRAW_CFG_DTYPE)
            for op, rng in enumerate(self.ranges):
                cfg["factor_lo"][0, op], cfg["factor_hi"][0, op] = rng if rng is not None else (1.0, 1.0)
            if self.translate is not None:
                cfg["max_dx"], cfg["max_dy"] = float(self.translate[0] * w), float(self.translate[1] * h)
            cfg["scale_lo"], cfg["scale_hi"] = self.scale if self.scale is not None else (1.0, 1.0)
            if self.erase is not None:
                cfg["erase"], cfg["p"] = 1, self.erase.p
                cfg["prop_lo"], cfg["prop_hi"] = self.erase.proportion
                cfg["dot_lo"], cfg["dot_hi"] = self.erase.dot_size
            self._cfgs[(h, w)] = cfg
        return cfg

    def draw_device(self, n: int, h: int, w: int, device) -> DeviceDraws:
        """The draws for n images of h x w made by one launch on ``device``'s current stream (mvg_augment_draw): nothing is
        built on the host but the settings struct (cached per size), nothing is copied, nothing synchronises.  Launch k of
        this object (the device counter) draws image i from Philox4x32-10(key = seed, counter = (i, block, k))."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("TrainAugment (MI355X build) draws on the device: no CPU fallback")
        if self.draws != "device":
            raise RuntimeError("TrainAugment.draw_device needs draws='device' (and a seed)")
        if self._counter is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("TrainAugment: the launch counter must exist before a capture (run one eager step first: "
                                   "graph.GraphedStep's warm-up does)")
            self._counter = torch.full((1,), self._counter_start, dtype=torch.int64, device=device)
        elif self._counter.device != device:
            raise RuntimeError(f"TrainAugment: the launch counter lives on {self._counter.device}, the batch on {device}")
        recs = torch.empty(n * REC_DTYPE.itemsize, dtype=torch.uint8, device=device)
        masks = grid = None
        if self.erase is not None:
            masks = torch.empty(n, self._gmax * self._gmax, dtype=torch.float32, device=device)
            grid = torch.empty(n, dtype=torch.int32, device=device)
        ops.augment_draw(recs, masks, grid, self._gmax, n, h, w, self._draw_cfg(h, w), self.seed, self._counter)
        return DeviceDraws(recs, masks, grid, self._gmax)

    def state_dict(self) -> dict:
        """{"seed", "counter"}: what reproduces the device draws from here on (reads the device counter: may synchronise)."""
        counter = self._counter_start if self._counter is None else int(self._counter.item())
        return {"seed": self.seed, "counter": counter & ((1 << 64) - 1)}

    def load_state_dict(self, state: dict) -> None:
        """Take seed and counter back.  The counter is written IN PLACE: a captured step holds the tensor's address."""
        seed, counter = state["seed"], int(state["counter"]) & ((1 << 64) - 1)
        if self.draws == "device" and (isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64):
            raise ValueError(f"draws='device' needs seed = an int of at most 64 bits (got {seed!r})")
        if self._counter is not None and seed != self.seed:
            raise ValueError("TrainAugment: the seed travels by value in queued and captured launches and cannot change once the "
                             "device draws have started: build a new TrainAugment")
        self.seed = seed
        self._counter_start = counter - (1 << 64) if counter >= 1 << 63 else counter       # the int64 bit pattern
        if self._counter is not None:
            self._counter.copy_(torch.full((1,), self._counter_start, dtype=torch.int64))

    def draw(self, n: int, h: int, w: int) -> AugmentDraws:
        """The host draws for n images of h x w, image by image, in the order torchvision's transforms make them - restated
        from torchvision's source as documented (ColorJitter.get_params / forward, RandomAffine.get_params), NOT pinned by a
        fixture: torchvision is not a dependency of the tests; only the pixel arithmetic is pinned.  Per image:
        ``torch.randperm(4)`` (index 3 is hue: skipped), ``torch.empty(1).uniform_`` for the brightness, contrast and
        saturation factors (an op whose range is [1, 1] draws nothing and is the identity), the affine angle (drawn from
        [0, 0], consumed), ``tx = int(round(uniform(-translate[0]*w, translate[0]*w)))``, ``ty`` likewise with h, the
        scale, then RandomMultiErasing.draw's calls for that image."""
        recs = np.zeros(n, dtype=REC_DTYPE)
        erase: Optional[List[Tuple[int, Tensor]]] = [] if self.erase is not None else None
        for i in range(n):
            perm = torch.randperm(4).tolist()
            recs["order"][i] = [op for op in perm if op != 3]
            for op, rng in enumerate(self.ranges):
                recs["factor"][i, op] = 1.0 if rng is None else float(torch.empty(1).uniform_(rng[0], rng[1]))
            float(torch.empty(1).uniform_(0.0, 0.0).item())                 # the angle
            tx = ty = 0
            if self.translate is not None:
                max_dx, max_dy = float(self.translate[0] * w), float(self.translate[1] * h)
                tx = int(round(torch.empty(1).uniform_(-max_dx, max_dx).item()))
                ty = int(round(torch.empty(1).uniform_(-max_dy, max_dy).item()))
            scale = 1.0
            if self.scale is not None:
                scale = float(torch.empty(1).uniform_(self.scale[0], self.scale[1]).item())
            recs["a0"][i], recs["cx"][i], recs["a4"][i], recs["cy"][i] = inverse_affine(h, w, scale, tx, ty)
            if erase is not None:
                erase += self.erase.draw(1)
        return AugmentDraws(recs, erase)

    def launch(self, u8: Tensor, draws, dst_u8: Optional[Tensor], dst_nhwc4: Optional[Tensor], bgr: bool = False, *,
               dst_nhwc8: Optional[Tensor] = None, dst_rw: Optional[Tensor] = None) -> None:
        """One launch into caller-owned destinations (uint8 [n, h, w, 3] and / or fp32 [n, h, w, 4]); one host-to-device copy
        carries the records (and, with erase draws, one each the masks and grid sizes).  dst_nhwc8 (bf16 [n, h, w, 8]) and /
        or dst_rw (bf16 [n, h, w/4, 64], the bf16 stem's row windows: w % 4 == 0): the same launch straight into the bf16
        stem's operand (mvg_augment_u8hwc_bf16), the fp32 value rounded once; not together with dst_u8 / dst_nhwc4.
        draws: an AugmentDraws, or a DeviceDraws (draw_device) - already in device memory: no copy, no host check of the records."""
        bf16 = dst_nhwc8 is not None or dst_rw is not None
        if bf16 and (dst_u8 is not None or dst_nhwc4 is not None):
            raise ValueError("TrainAugment: bf16 destinations (dst_nhwc8, dst_rw) and dst_u8 / dst_nhwc4 take a launch each")
        if not u8.is_cuda:
            raise RuntimeError("TrainAugment (MI355X build) works on device batches: no CPU fallback")
        if u8.dim() != 4 or u8.shape[3] != 3 or u8.dtype != torch.uint8:
            raise ValueError(f"TrainAugment: expected uint8 [n, h, w, 3] patches (got {u8.dtype} {tuple(u8.shape)})")
        n, h, w, _ = u8.shape
        if dst_rw is not None and w % 4:
            raise ValueError(f"TrainAugment: the bf16 row windows need a width that is a multiple of 4 (got {w})")
        if isinstance(draws, DeviceDraws):
            if draws.recs.numel() != n * REC_DTYPE.itemsize:
                raise ValueError(f"TrainAugment: {draws.recs.numel() // REC_DTYPE.itemsize} records for {n} images")
            if draws.masks is not None and dst_nhwc4 is None and not bf16:
                raise ValueError("TrainAugment: the erase multiplies the normalised image: out='u8' needs erase=None")
            aug = ops.augment_u8hwc_bf16 if bf16 else ops.augment_u8hwc
            aug(u8.contiguous(), draws.recs, *((dst_nhwc8, dst_rw) if bf16 else (dst_u8, dst_nhwc4)), draws.masks, draws.grid, draws.gmax,
                n, h, w, IMAGE_MEAN, IMAGE_STD, bgr, recs_host=None)
            return
        recs = np.ascontiguousarray(draws.recs, dtype=REC_DTYPE)
        if recs.shape != (n,):
            raise ValueError(f"TrainAugment: {recs.shape[0] if recs.ndim else 0} records for {n} images")
        masks = grid = None
        gmax = 0
        if draws.erase is not None and any(g for g, _ in draws.erase):
            if dst_nhwc4 is None and not bf16:
                raise ValueError("TrainAugment: the erase multiplies the normalised image: out='u8' needs erase=None")
            assert len(draws.erase) == n
            gmax = max(g for g, _ in draws.erase)
            mh, gh = torch.zeros(n, gmax * gmax, dtype=torch.float32), torch.zeros(n, dtype=torch.int32)
            for i, (g, m) in enumerate(draws.erase):
                gh[i] = g
                if g:
                    mh[i, : g * g] = m.reshape(-1)
            masks, grid = mh.to(u8.device), gh.to(u8.device)
        dev_recs = torch.from_numpy(recs.view(np.uint8).reshape(-1)).to(u8.device)
        if bf16:
            ops.augment_u8hwc_bf16(u8.contiguous(), dev_recs, dst_nhwc8, dst_rw, masks, grid, gmax, n, h, w, IMAGE_MEAN, IMAGE_STD, bgr,
                                   recs_host=recs)
        else:
            ops.augment_u8hwc(u8.contiguous(), dev_recs, dst_u8, dst_nhwc4, masks, grid, gmax, n, h, w, IMAGE_MEAN, IMAGE_STD, bgr,
                              recs_host=recs)

    def apply(self, u8: Tensor, draws, out: str = "nhwc4", bgr: bool = False) -> Tensor:
        """u8 [n, h, w, 3] uint8 on the GPU (bgr: stored BGR) -> ``"nhwc4"``: fp32 [n, h, w, 4], the backbone's input layout
        (channel 3 zero); ``"nchw"``: fp32 [n, 3, h, w], the reference transform's output format (for callers outside the
        model); ``"u8"``: uint8 [n, h, w, 3] RGB, the image before ToTensor (no erase); ``"nhwc8_bf16"``: bf16 [n, h, w, 8],
        the nhwc4 values rounded once, channels 3..7 zero; ``"rw_bf16"``: bf16 [n, h, w/4, 64], the bf16 stem's row windows of
        that image (ops.stem_rowwindow_bf16's layout; w % 4 == 0) - the two operands of the bf16 stem, one launch each."""
        if out not in ("nhwc4", "u8", "nchw", "nhwc8_bf16", "rw_bf16"):
            raise ValueError(f"out must be 'nhwc4', 'u8', 'nchw', 'nhwc8_bf16' or 'rw_bf16' (got {out!r})")
        if not u8.is_cuda:
            raise RuntimeError("TrainAugment (MI355X build) works on device batches: no CPU fallback")
        n, h, w = u8.shape[:3]
        if out == "rw_bf16":
            if w % 4:
                raise ValueError(f"out='rw_bf16': the bf16 row windows need a width that is a multiple of 4 (got {w})")
            dst = torch.empty(n, h, w // 4, 64, dtype=torch.bfloat16, device=u8.device)
            self.launch(u8, draws, None, None, bgr, dst_rw=dst)
            return dst
        if out == "nhwc8_bf16":
            dst = torch.empty(n, h, w, 8, dtype=torch.bfloat16, device=u8.device)
            self.launch(u8, draws, None, None, bgr, dst_nhwc8=dst)
            return dst
        if out == "u8":
            dst = torch.empty(n, h, w, 3, dtype=torch.uint8, device=u8.device)
            self.launch(u8, draws, dst, None, bgr)
            return dst
        x = torch.empty(n, h, w, 4, dtype=torch.float32, device=u8.device)
        self.launch(u8, draws, None, x, bgr)
        if out == "nhwc4":
            return x
        y = torch.empty(n, 3, h, w, dtype=torch.float32, device=u8.device)
        ops.nhwc4_to_nchw(x, y, n, 3, h, w)
        return y

    def __call__(self, u8: Tensor, out: str = "nhwc4", bgr: bool = False) -> Tensor:
        n, h, w = u8.shape[:3]
        return self.apply(u8, self.draw_device(n, h, w, u8.device) if self.capturable else self.draw(n, h, w), out, bgr)
