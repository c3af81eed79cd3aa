"""The inference range guard on the GPU: the ranged split kernels, the Python guard, the session's record, graph capture.

The record: one 32-bit word per sp tensor = max over the stored elements of the BITS of |v| (an unsigned-integer atomic max:
monotone for non-negative floats, inf / NaN on top), v the fp32 value handed to the fp16 split.  Over iff the word is
>= 0x477FF000 (65520.0f: where fp16 round-to-nearest-even gives inf).  Everything here is a condition, not a tolerance: the
ranged kernels store the unranged kernels' bits (torch.equal) and the word is the bit pattern of max |twin|, twin being the
fp32-output launch of the EXISTING entry point on the same inputs (same accumulators, same epilogue arithmetic).

Which instantiation a shape runs is decided on the host (split_plan): every kernel case first asserts, through the host-only
plan queries, that it runs the form it is here for - as tests/test_split_forms_gpu.py does with ops.set_reserved_cus:
  * K-loop stages: mvg_conv_fprop_split_stages (two stages exist for 128 x 128 tiles only);
  * column tile: 128 columns from cout >= 128, else 64;
  * row-tile height: 256 when the GEMM has fewer than 128 columns, more than one tap and at least 65 536 rows, else 128.  No
    host query returns it for a forward, but mvg_conv_dgrad_bn_partials_split sizes its partials with the same function of
    (columns, taps, rows): asked about the stride-1 descriptor whose backward-data GEMM has this forward's columns and rows
    it returns ceil(rows / tile height).
"""
import contextlib

import numpy as np
import pytest
import torch

import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd import synth

pytestmark = pytest.mark.gpu

OVER = 0x477FF000                       # bits of 65520.0f
BELOW = 0x477FEFFF                      # the largest fp32 below 65520
HUGE = 0x7F000000                       # a finite value no test reaches: a pre-set word must survive


def dev():
    return torch.device("cuda:0")


def f32_from_bits(bits):
    return float(np.array([bits], dtype=np.uint32).view(np.float32)[0])


def bits_of_absmax(t):
    return int(t.abs().max().reshape(1).view(torch.int32).item())


def word(value=0):
    return torch.full((1,), value, dtype=torch.int32, device=dev())


@contextlib.contextmanager
def reserved_cus(n):
    from rot_mvgaze_amd import ops
    try:
        ops.set_reserved_cus(n)
        yield
    finally:
        ops.set_reserved_cus(0)


def desc(case):
    from rot_mvgaze_amd._lib import ConvDesc
    G, N, h, cin, cout, k, st, pad = case
    return ConvDesc.make(G, N, h, h, cin, cout, k, st, pad)


def tile_rows_of(case):
    """Row-tile height of the forward launch of ``case`` (see the module docstring)."""
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import ConvDesc
    G, N, h, cin, cout, k, st, pad = case
    d = desc(case)
    rows = N * d.ho * d.wo
    twin = ConvDesc.make(G, N, d.ho, d.wo, cout, cin, k, 1, (k - 1) // 2)     # its backward-data GEMM: cout columns, this forward's rows
    assert (twin.h, twin.w, twin.cin) == (d.ho, d.wo, cout)
    parts = ops.conv_dgrad_bn_partials_split(twin)
    fits = [t for t in (128, 256) if parts == -(-rows // t)]
    assert fits, f"{parts} partials for {rows} rows: neither 128- nor 256-row tiles"
    return fits[0]          # (a map of at most 128 rows is one tile either way: far below the 65 536 rows the taller tile asks for)


# (G, N, h, cin, cout, k, stride, pad), CUs left to the planners (None: all), the form: (column tile, row tile, stages)
KERNEL_CASES = [
    ((1, 2, 8, 32, 64, 1, 1, 0), None, (64, 128, 1)),             # 64 columns: igemm_split16_ranged_kernel<64>
    ((1, 10, 15, 96, 160, 1, 1, 0), None, (128, 128, 2)),         # ragged last row tile, ragged second column tile: <128, 2, 2>
    ((1, 10, 15, 96, 160, 1, 1, 0), 8, (128, 128, 1)),            # ... and <128>
    ((2, 6, 14, 256, 256, 3, 1, 1), None, (128, 128, 2)),         # 40 tiles, 72 K-steps: two-stage <128, 2, 2>
    ((2, 6, 14, 256, 256, 3, 1, 1), 8, (128, 128, 1)),            # single-stage <128>
    ((1, 21, 56, 64, 64, 3, 1, 1), None, (64, 256, 1)),           # 65 856 rows: the 256 x 64 tile <64, 4>
]
RAGGED = KERNEL_CASES[1]


def kid(kc):
    case, cus, form = kc
    return "g%d_n%d_h%d_%dto%d_k%d_s%d_p%d" % case + ("_allcus" if cus is None else f"_{cus}cus") + "_bn%d_bm%d_st%d" % form


@contextlib.contextmanager
def planned(kc):
    """The planners' CU budget of a kernel case, with the form asserted from the host."""
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import lib
    case, cus, (bn, bm, stages) = kc
    total = lib().mvg_device_cus()
    assert total >= 64, "the form guards are written for a device with many more than 8 CUs"
    with reserved_cus(0 if cus is None else total - cus):
        d = desc(case)
        assert (128 if d.cout >= 128 else 64) == bn
        assert ops.conv_fprop_split_stages(d) == stages, f"{kid(kc)}: no longer the {stages}-stage K loop"
        assert tile_rows_of(case) == bm, f"{kid(kc)}: no longer {bm}-row tiles"
        yield d


class Inputs:
    def __init__(self, case, zero_weights=False):
        from rot_mvgaze_amd import ops
        G, N, h, cin, cout, k, st, pad = case
        torch.manual_seed(sum(case))
        self.d = d = desc(case)
        x = torch.relu(torch.randn(G, N, h, h, cin, device=dev()))
        w = torch.randn(cout, k, k, cin, device=dev()) * (1.0 / (k * k * cin) ** 0.5)
        if zero_weights:
            w.zero_()
        self.xs = ops.split_f32(x)
        self.wk, _ = ops.split_weights(d, w, False)
        self.scale = torch.rand(cout, device=dev()) + 0.5
        self.shift = torch.randn(cout, device=dev()) * 0.5
        self.residual = torch.randn(G, N, d.ho, d.wo, cout, device=dev())
        self.shape = (G, N, d.ho, d.wo, cout)

    def unranged(self, residual, scale=None, shift=None):
        from rot_mvgaze_amd import ops
        out = ops.sp_empty(*self.shape, device=dev())
        out.fill_(float("nan"))
        ops.conv_fprop_split_affine(self.d, self.xs, self.wk, out, self.scale if scale is None else scale,
                                    self.shift if shift is None else shift, residual, True)
        return out

    def twin(self, residual):
        from rot_mvgaze_amd import ops
        out = torch.full(self.shape, float("nan"), device=dev())
        ops.conv_fprop_split_affine(self.d, self.xs, self.wk, out, self.scale, self.shift, residual, True)
        return out

    def ranged(self, residual, w, scale=None, shift=None):
        from rot_mvgaze_amd import ops
        out = ops.sp_empty(*self.shape, device=dev())
        out.fill_(float("nan"))
        ops.conv_fprop_split_affine_ranged(self.d, self.xs, self.wk, out, self.scale if scale is None else scale,
                                           self.shift if shift is None else shift, residual, True, w)
        return out


# ---------------------------------------------------------------- 1. the ranged conv kernels
@pytest.mark.parametrize("with_residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("kc", KERNEL_CASES, ids=[kid(k) for k in KERNEL_CASES])
def test_ranged_conv_same_bits_and_exact_word(kc, with_residual):
    inp = Inputs(kc[0])
    res = inp.residual if with_residual else None
    with planned(kc):
        want = inp.unranged(res)
        twin = inp.twin(res)
        w0, w1 = word(0), word(HUGE)
        got0 = inp.ranged(res, w0)
        got1 = inp.ranged(res, w1)
    assert torch.isfinite(twin).all() and float(twin.max()) > 0
    # (a) the stored bits are the unranged kernel's
    assert torch.equal(got0.view(torch.int16), want.view(torch.int16)) and torch.equal(got1.view(torch.int16), want.view(torch.int16))
    # (b) the word is the bit pattern of max |twin|
    print(f"RANGE {kid(kc)} residual={with_residual}: word {int(w0.item()):#010x} = {f32_from_bits(int(w0.item())):.6g}, "
          f"max |twin| {float(twin.abs().max()):.6g}")
    assert int(w0.item()) == bits_of_absmax(twin)
    assert int(w0.item()) < OVER
    # (c) a larger word is left alone
    assert int(w1.item()) == HUGE


def test_threshold_is_exact():
    """Zero weights, scale 1: the output is relu(shift).  0x477FEFFF is not over and merges to a finite tensor; 65520.0 is over."""
    from rot_mvgaze_amd import ops
    kc = KERNEL_CASES[0]
    inp = Inputs(kc[0], zero_weights=True)
    cout, c0 = inp.d.cout, 5
    scale = torch.ones(cout, device=dev())
    for bits, over in ((BELOW, False), (OVER, True)):
        shift = torch.zeros(cout, device=dev())
        shift[c0] = f32_from_bits(bits)
        assert int(shift[c0:c0 + 1].view(torch.int32).item()) == bits
        w = word(0)
        with planned(kc):
            out = inp.ranged(None, w, scale, shift)
            want = inp.unranged(None, scale, shift)
        assert torch.equal(out.view(torch.int16), want.view(torch.int16))
        assert int(w.item()) == bits and (int(w.item()) >= OVER) == over
        merged = ops.merge_sp(out)
        if over:
            assert not torch.isfinite(merged[..., c0]).any()          # inf in the high piece, NaN after the merge: what the word reports
        else:
            # (the two pieces keep 22 of the 24 significand bits here: 65504 + 16 - within 2^-23 of the value, as the format promises)
            a = f32_from_bits(BELOW)
            assert torch.isfinite(merged).all() and abs(float(merged.max()) - a) <= a * 2.0 ** -23
            assert float(merged[..., c0].min()) == float(merged.max())


@pytest.mark.parametrize("kc", [RAGGED, KERNEL_CASES[2]], ids=[kid(RAGGED), kid(KERNEL_CASES[2])])
def test_last_valid_row_and_column_count_and_nothing_beyond(kc):
    """One residual element in the LAST valid row and LAST valid column of the ragged case: 1e5 there is over, 6e4 is not - so the
    corner takes part, and nothing beyond the map's edge (the ragged tiles' other rows and columns) does."""
    inp = Inputs(kc[0])
    for value, over in ((1e5, True), (6e4, False)):
        res = torch.zeros(inp.shape, device=dev())
        res[-1, -1, -1, -1, -1] = value
        w = word(0)
        with planned(kc):
            out = inp.ranged(res, w)
            twin = inp.twin(res)
            want = inp.unranged(res)
        assert torch.equal(out.view(torch.int16), want.view(torch.int16))
        print(f"RANGE corner {kid(kc)} {value:g}: word {f32_from_bits(int(w.item())):.6g}")
        assert int(w.item()) == bits_of_absmax(twin)
        assert (int(w.item()) >= OVER) == over
        assert float(twin[-1, -1, -1, -1, -1]) == float(twin.max()) >= value - 100.0


# ---------------------------------------------------------------- 2. split_f32 with the record
@pytest.mark.parametrize("n", [8, 8 * 1000 + 8])
def test_split_f32_ranged(n):
    from rot_mvgaze_amd import ops
    torch.manual_seed(n)
    x = torch.randn(n, device=dev()) * 3.0
    want = ops.split_f32(x)
    w0, w1 = word(0), word(HUGE)
    got0, got1 = ops.split_f32_ranged(x, w0), ops.split_f32_ranged(x, w1)
    assert torch.equal(got0.view(torch.int16), want.view(torch.int16)) and torch.equal(got1.view(torch.int16), want.view(torch.int16))
    assert int(w0.item()) == bits_of_absmax(x) and int(w1.item()) == HUGE
    # the threshold pair, on the LAST element (negative: the record is of |v|)
    for bits, over in ((BELOW, False), (OVER, True)):
        y = x.clone()
        y[-1] = -f32_from_bits(bits)
        w = word(0)
        out = ops.split_f32_ranged(y, w)
        assert torch.equal(out.view(torch.int16), ops.split_f32(y).view(torch.int16))
        assert int(w.item()) == bits and (int(w.item()) >= OVER) == over
        assert bool(torch.isfinite(ops.merge_sp(out)).all()) == (not over)
    # a scale takes part: the record is of the stored value x * scale
    w = word(0)
    ops.split_f32_ranged(x, w, 2.0 ** 10)
    assert int(w.item()) == bits_of_absmax(x * 2.0 ** 10)
    # inf and NaN rank above every finite value (fmaxf would drop the NaN)
    for bad in (float("inf"), float("nan")):
        y = x.clone()
        y[0] = bad
        w = word(0)
        ops.split_f32_ranged(y, w)
        assert int(w.item()) >= 0x7F800000


# ---------------------------------------------------------------- 3. the model
UNIT = "_feat_extractor.0.layer2.0.conv1"
_MODELS = {}


def _model(depth, fresh=False):
    from rot_mvgaze_amd.model import FeatRotationSymm
    if fresh or depth not in _MODELS:
        sd = synth.make_state_dict(depth, 0, 3, perturb_bn=True)
        m = FeatRotationSymm(depth, 3)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
        m.to(dev()).eval()
        m.ensure_layout()
        if fresh:
            return m
        _MODELS[depth] = m
    return _MODELS[depth]


def _perturbed():
    """ResNet-18 whose layer2.0.conv1 unit writes ~1e5: past fp16's range."""
    m = _model(18, fresh=True)
    with torch.no_grad():
        dict(m.named_parameters())["_feat_extractor.0.layer2.0.bn1.bias"].add_(1e5)
    return m


def _inputs(B=2, V=2, hw=64, seed=1234):
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    inp = synth.make_inputs(B, V, seed, hw)
    img, hp = torch.from_numpy(inp["img"]), torch.from_numpy(inp["head_pose"])
    imgs = [img[:, v].contiguous().to(dev()) for v in range(V)]
    rot = torch.stack([rotation_matrix_2d(hp[:, v].contiguous().to(dev())) for v in range(V)], dim=1).contiguous()
    return imgs, rot


def _run(m, imgs, rot, guard):
    m.split_eval_guard = guard
    with torch.no_grad():
        out = m.run_views(imgs, rot)
    return [o.detach().clone() for o in out]


def _same(got, want):
    for n, a, b in zip(("img_feat", "lifted", "feats", "preds"), got, want):
        assert torch.isfinite(b).all(), n
        assert torch.equal(a, b), f"{n}: max |diff| {(a - b).abs().max().item():.3e}"


@pytest.fixture(scope="module")
def clean18():
    """(model, inputs, outputs with the guard off) of ResNet-18, V = 2, B = 2, 64 px - computed once."""
    m = _model(18)
    assert m._backbone.split and m._backbone.split_eval
    imgs, rot = _inputs()
    return m, imgs, rot, _run(m, imgs, rot, None)


@pytest.mark.parametrize("guard", ["record", "fallback"])
def test_guard_keeps_the_outputs_of_a_clean_checkpoint(clean18, guard):
    from rot_mvgaze_amd.arch import range_unit_names
    m, imgs, rot, want = clean18
    try:
        _same(_run(m, imgs, rot, guard), want)
        assert m.overflowed() == []
        rep = m.range_report()
        assert list(rep) == range_unit_names(18) and len(rep) == 17
        assert all(0.0 < v < 65520.0 for v in rep.values()), rep
        assert not m._backbone._range_tripped
        assert not any("range" in k for k in m.state_dict())
    finally:
        m.split_eval_guard = None
    _same(_run(m, imgs, rot, None), want)


def test_record_names_the_first_overflowing_unit():
    m = _perturbed()
    imgs, rot = _inputs()
    _run(m, imgs, rot, "record")
    over = m.overflowed()
    assert over and over[0] == UNIT, over
    rep = m.range_report()
    assert rep[UNIT] >= 65520.0 and all(v < 65520.0 for n, v in rep.items() if n == "_feat_extractor.0.conv1" or ".layer1." in n)


def test_fallback_reruns_on_the_fp32_kernels_and_stays_there():
    m = _perturbed()
    imgs, rot = _inputs()
    bb = m._backbone
    bb.split_eval = False
    want = _run(m, imgs, rot, None)                     # the same model with split_eval = False
    bb.split_eval = True
    _same(_run(m, imgs, rot, "fallback"), want)
    assert m.overflowed()[0] == UNIT and bb._range_tripped      # the record of the split pass says why
    # the next call launches no split conv: with the guard on every one of them would write its word
    _same(_run(m, imgs, rot, "fallback"), want)
    assert m.overflowed() == [] and all(v == 0.0 for v in m.range_report().values())
    assert bb._range_tripped
    # new weights re-arm it
    m.invalidate_weight_cache()
    assert not bb._range_tripped
    _same(_run(m, imgs, rot, "fallback"), want)
    assert m.overflowed()[0] == UNIT and bb._range_tripped
    # and the other guards are not affected by the latch
    _run(m, imgs, rot, "record")
    assert m.overflowed()[0] == UNIT


def test_resnet50_clean_pass():
    from rot_mvgaze_amd.arch import range_unit_names
    m = _model(50)
    imgs, rot = _inputs()
    want = _run(m, imgs, rot, None)
    try:
        _same(_run(m, imgs, rot, "record"), want)
        assert m.overflowed() == [] and list(m.range_report()) == range_unit_names(50)
        assert all(0.0 < v < 65520.0 for v in m.range_report().values())
    finally:
        m.split_eval_guard = None


def test_guard_rejects_an_unknown_setting(clean18):
    m, imgs, rot, _ = clean18
    try:
        with pytest.raises(ValueError):
            _run(m, imgs, rot, "on")
    finally:
        m.split_eval_guard = None


# ---------------------------------------------------------------- 4. the session
def test_session_record_matches_the_python_backbone(clean18):
    from rot_mvgaze_amd.arch import range_unit_names
    from rot_mvgaze_amd.session import InferenceSession
    m, imgs, rot, want = clean18
    try:
        _run(m, imgs, rot, "record")
        py_words = m._backbone._range_record.clone()
    finally:
        m.split_eval_guard = None
    with InferenceSession(m, 2, 2, 64, 64) as plain, InferenceSession(m, 2, 2, 64, 64, range_record=True) as s:
        assert s.launches == plain.launches and s.range_unit_names == range_unit_names(18)
        _same(plain.run(imgs, rot), want)
        _same(s.run(imgs, rot), want)
        assert torch.equal(s._range_record, py_words)
        assert s.overflowed() == [] and list(s.range_report()) == range_unit_names(18)
        _same(s.run(imgs, rot), want)                   # the record is cleared per forward: a second run leaves the same words
        assert torch.equal(s._range_record, py_words)
        with pytest.raises(RuntimeError):
            plain.overflowed()


def test_session_reports_the_overflowing_unit():
    from rot_mvgaze_amd.session import InferenceSession
    m = _perturbed()
    imgs, rot = _inputs()
    _run(m, imgs, rot, "record")
    py_over, py_words = m.overflowed(), m._backbone._range_record.clone()
    m.split_eval_guard = None
    with InferenceSession(m, 2, 2, 64, 64, range_record=True) as s:
        s.run(imgs, rot)
        assert s.overflowed() == py_over and s.overflowed()[0] == UNIT
        assert torch.equal(s._range_record, py_words)


# ---------------------------------------------------------------- 5. graph capture
def test_record_guard_is_capturable_and_fallback_is_not(clean18):
    m, imgs, rot, want = clean18
    side = torch.cuda.Stream(device=dev())
    try:
        m.split_eval_guard = "record"
        side.wait_stream(torch.cuda.current_stream(dev()))
        with torch.cuda.stream(side), torch.no_grad():          # warm-up: allocator pools, weight copies, the record tensor
            for _ in range(2):
                m.run_views(imgs, rot)
        torch.cuda.current_stream(dev()).wait_stream(side)
        torch.cuda.synchronize(dev())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side), torch.no_grad():  # one stream, no side streams: a graph without parallel branches
            out = m.run_views(imgs, rot)
        for o in out:
            o.zero_()
        m._backbone._range_record.fill_(-1)
        g.replay()
        torch.cuda.synchronize(dev())
        _same([o.clone() for o in out], want)
        assert m.overflowed() == [] and all(0.0 < v < 65520.0 for v in m.range_report().values())
        # "fallback" reads the record on the host: refused while the stream is capturing, before anything is queued
        m.split_eval_guard = "fallback"
        g2 = torch.cuda.CUDAGraph()
        marker = torch.zeros(8, device=dev())
        with pytest.raises(RuntimeError, match="capturing"):
            with torch.cuda.graph(g2, stream=side), torch.no_grad():
                marker.add_(1.0)                                # (the capture is not empty)
                m.run_views(imgs, rot)
        torch.cuda.synchronize(dev())
    finally:
        m.split_eval_guard = None
    _same(_run(m, imgs, rot, None), want)
