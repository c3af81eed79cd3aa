"""The operand producers every conv launch depends on - mvg_split_f32 / _ranged / mvg_merge_sp, mvg_weights_prep_batch in both
modes with several records per launch, the three row-window builders - and the stems' row-window conv forms
(mvg_stem_fprop_split / _wgrad_split / _fprop_bf16 / _wgrad_bf16), at kernel level.  tests/prep_forms_ref.py holds the host
references and the case tables, tests/test_prep_forms_cpu.py checks those on their own.

Conventions of test_bf16_forms_gpu.py: every output starts as NaN (the range word and the stat pairs as the zero their
contract asks for) inside a larger allocation whose sentinel margins on both sides must be bit-unchanged afterwards (`Guarded`);
every stem case FIRST asserts, through the host-only queries mvg_stem_plan_query_split / _bf16 (answered by the code the
launches plan with), which form it is about to run, and the last test holds the union of the forms seen to prep_forms_ref.FORMS;
every comparison prints its figure as `PREP-FORMS <case> <form>: ...` before it asserts.

Conditions - none fitted to the kernels:
  sp stores (A, B mode 1, C): the device's pieces equal prep_forms_ref.sp_pieces of the stored values bit for bit.  One
      exception: an element whose reference second piece is a nonzero fp16 subnormal may differ, must then still satisfy
      |merged - stored| <= 2^-23 |stored| + 2^-25, and such elements are counted, printed and at most 0.1 % of the tensor.
      (The bound admits the other neighbour of a tie, not a piece flushed to zero: tests/test_prep_forms_cpu.py.)
  merge: bit-equal to (h1 + h2) * inv_scale in fp32.  The range word: the integer maximum of the bits of |x * scale|, exactly.
  weight prep: mode 1 stat[0] = the bits of max |w|, stat[1] = 1 / sp_scale_for(max) exactly, both copies under the sp condition,
      the same bits whatever the record's neighbours, workgroup count and order; mode 0 bit-equal to w.to(bfloat16), padding zero.
  row windows: the sp condition / bit equality against the host gather.
  split stem: y and dw within SPLIT_VS_F64 / SPLIT_VS_FP32_KERNEL of float64 conv2d next to the fp32-MFMA kernel on the same
      inputs AND per element close(.., 2e-5); every statistics partial on its own against float64 over exactly its rows (sum
      1e-4, centred squares 1e-3, the bars of test_split_fprop_single_stage_and_pipelined); bits equal across the two K loops.
  bf16 stem: y per element within bf16_forms_ref.bf16_bound with M = max conv(|x|, |w|); dw close(.., 2e-5) after un-folding;
      every folded partial 2 pi + par against float64 over the pixels (n, oy, 2 m + par) of folded rows 64 pi .. 64 pi + 63 at
      2e-4 of the partial's largest; a run whose y is exactly 1 everywhere counts every output pixel exactly once.

Measured on an MI355X (profiles/prep_forms_errors.txt), smallest .. largest over the cases (the bars above were not refitted to them):
  sp stores, 91 comparisons (split_f32 / _ranged at 8 .. 16 777 240 elements, both copies of every mode-1 record, the row windows
      up to 33 x 256 x 256): elements differing from the host pieces 0 .. 0; subnormal-piece elements that differed 0 .. 0 - the
      device rounds fp16 subnormals as numpy does, so the exception was never used
  merge, range word, stat pairs, mode-0 copies, bf16 row windows: elements / words differing 0 .. 0
  split stem y, relative L2            1.3e-07 .. 1.7e-07 (fp32-MFMA kernel 1.6e-07 .. 2.1e-07), largest element error 2.2e-07 .. 4.2e-07 of max |ref|
  split stem dw, relative L2           2.7e-08 .. 6.0e-07 (fp32-MFMA kernel 9.2e-08 .. 3.0e-07), largest element error 5.9e-08 .. 1.1e-06
  split stem partials, of their bars   sum 5.5e-04 .. 1.1e-03, centred squares 1.9e-04 .. 3.4e-04
  bf16 stem y, largest bound ratio     0.942 .. 0.966;  folded partials 1.7e-07 .. 3.1e-07 of the partial's largest;  pixel counts exact
  bf16 stem dw, relative L2            5.6e-08 .. 1.5e-07, largest element error 8.3e-08 .. 2.6e-07 of max |ref|

What the cases taught.  The fp32-MFMA kernel takes power-of-two channel counts under a 7x7 filter, so the split stem at cout = 96
has no fp32-MFMA figure next to it: there SPLIT_VS_F64 and the per-element bar stand alone.  The bound of the sp exception
(2^-25 absolute) is half a subnormal spacing: it admits the other neighbour of a tie, never a flushed piece (a flush of a piece
near 2^-15 is off by a thousand times the bound) - on this device the question does not arise.  And weights_prep_batch_kernel
stores the second piece of a source -0.0 as -0.0 in the first two lanes of a chunk where fp16(v - h1) is +0.0 (mvg_split_f32
stores +0.0 in all eight): the sum of the pieces is a zero either way, and the all-zeros record is made of +0.0.
"""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import rot_mvgaze_amd  # noqa: F401
import bf16_forms_ref as B
import prep_forms_ref as R
from test_kernels_gpu import close, dev
from test_split_forms_gpu import reserved_cus, settings
from test_split_gpu import SPLIT_VS_F64, SPLIT_VS_FP32_KERNEL, rel_l2

pytestmark = pytest.mark.gpu

NAN = float("nan")
MARGIN = 4096                        # sentinel elements on either side of an output
_seen = set()
_subnormal_differences = []          # the exception's count per sp comparison


class Guarded:
    """An output tensor `.t` of `shape` inside a larger allocation: NaN (or `init`) inside, a bit pattern on both sides."""

    def __init__(self, shape, dtype=torch.float32, init=None):
        n = int(np.prod(shape)) if len(shape) else 1
        self.buf = torch.empty(n + 2 * MARGIN, dtype=dtype, device=dev())
        wide = self.buf.element_size() == 4
        self.ints = self.buf.view(torch.int32 if wide else torch.int16)
        self.sentinel = 0x5A5A5A5A if wide else 0x5A5A
        self.ints.fill_(self.sentinel)
        self.t = self.buf[MARGIN:MARGIN + n].view(shape)
        if init is None:
            self.t.fill_(NAN)                    # (fp16 0x7E00, bf16 0x7FC0: no store of a finite or infinite value gives them)
        elif isinstance(init, (int, float)):
            self.t.fill_(init)
        else:
            self.t.copy_(init)

    def intact(self, what):
        ok = bool((self.ints[:MARGIN] == self.sentinel).all()) and bool((self.ints[-MARGIN:] == self.sentinel).all())
        assert ok, f"{what}: the launch wrote outside its output"
        return self.t


def L():
    from rot_mvgaze_amd._lib import lib
    return lib()


def call(rc, what):
    from rot_mvgaze_amd._lib import check
    check(rc, what)


def p(t):
    from rot_mvgaze_amd import ops
    return ops._p(t)


def st():
    from rot_mvgaze_amd import ops
    return ops._s()


def u16(t):
    """A 2-byte device tensor's bits on the host."""
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def bits32(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def held_sp(out, stored, what):
    """The sp condition of the module docstring on `out` (a Guarded or a tensor of fp16 pieces) against the host pieces of `stored`."""
    got = out.intact(what) if isinstance(out, Guarded) else out
    assert got.dtype == torch.float16
    want = R.sp_pieces(stored)
    same = torch.equal(got.contiguous().view(torch.int16).view(-1), torch.from_numpy(want.view(np.int16).reshape(-1)).to(dev()))
    wrong, excused, worst = (0, 0, 0.0) if same else R.sp_compare(u16(got), stored)
    _subnormal_differences.append(excused)
    print(f"PREP-FORMS {what}: {stored.size} elements, differing outside the exception {wrong}, subnormal-piece elements that differ "
          f"{excused} (worst at {worst:.3f} of 2^-23 |v| + 2^-25)")
    assert wrong == 0, f"{what}: {wrong} elements differ from fp16(v), fp16(v - h1)"
    assert excused <= R.SUBNORMAL_SHARE * stored.size and worst <= 1.0, f"{what}: {excused} excused elements, worst {worst:.3f}"


def free():
    gc.collect()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- A. split / ranged split / merge
@pytest.mark.parametrize("scale_case", R.SPLIT_SCALES, ids=[s[0] for s in R.SPLIT_SCALES])
@pytest.mark.parametrize("n", R.SPLIT_SIZES)
def test_prep_forms_split_ranged_merge(n, scale_case):
    name, mag, scale = scale_case
    what = f"n={n} scale={name}"
    x = R.split_values(n, mag)
    stored = x * np.float32(scale)
    xd = torch.from_numpy(x).to(dev())
    out = Guarded((n // 8, 2, 8), torch.float16)
    call(L().mvg_split_f32(p(xd), p(out.t), n, scale, st()), "split_f32")
    held_sp(out, stored, f"{what} split_f32")
    out2, word = Guarded((n // 8, 2, 8), torch.float16), Guarded((1,), torch.int32, init=0)
    call(L().mvg_split_f32_ranged(p(xd), p(out2.t), n, scale, p(word.t), st()), "split_f32_ranged")
    assert torch.equal(out2.intact(what + " ranged").view(torch.int16), out.t.view(torch.int16)), what + ": the ranged kernel stores other bits"
    got_word, want_word = int(word.intact("range word").item()), R.range_word(stored)
    print(f"PREP-FORMS {what} split_f32_ranged: range word {got_word:#010x} (host {want_word:#010x})")
    assert got_word == want_word and want_word < R.RANGE_OVER_BITS
    merged = Guarded((n,))
    call(L().mvg_merge_sp(p(out.t), p(merged.t), n, 1.0 / scale, st()), "merge_sp")
    want = R.sp_merge(u16(out.t).reshape(n // 8, 2, 8), 1.0 / scale)
    differ = int((bits32(merged.intact(what + " merge")) != want.view(np.uint32)).sum())
    print(f"PREP-FORMS {what} merge_sp: elements differing from (h1 + h2) * inv_scale {differ}")
    assert differ == 0
    del xd, out, out2, merged
    if n > 1 << 20:
        free()


def test_prep_forms_range_word_trips_past_fp16():
    n = 8 * 257
    x = R.split_values(n, 1.0)
    x[1000], x[1500] = 70000.0, -65519.0                 # past 65504: the first overflows fp16, the second still rounds to 65504
    xd = torch.from_numpy(x).to(dev())
    out, word = Guarded((n // 8, 2, 8), torch.float16), Guarded((1,), torch.int32, init=0)
    call(L().mvg_split_f32_ranged(p(xd), p(out.t), n, 1.0, p(word.t), st()), "split_f32_ranged")
    got = int(word.intact("range word").item())
    print(f"PREP-FORMS n={n} over-range split_f32_ranged: range word {got:#010x} (threshold {R.RANGE_OVER_BITS:#010x})")
    assert got == R.range_word(x) == int(np.float32(70000.0).view(np.uint32)) and got >= R.RANGE_OVER_BITS
    held_sp(out, x, f"n={n} over-range split_f32_ranged")
    assert u16(out.t).reshape(-1, 2, 8)[125, 0, 0] == 0x7C00, "70000 stores an infinite first piece: what the threshold reports"


def test_prep_forms_empty_tensors_write_nothing():
    xd = torch.ones(8, device=dev())
    out, word, merged = Guarded((1, 2, 8), torch.float16), Guarded((1,), torch.int32, init=0), Guarded((8,))
    assert L().mvg_split_f32(p(xd), p(out.t), 0, 1.0, st()) == 0
    assert L().mvg_split_f32_ranged(p(xd), p(out.t), 0, 1.0, p(word.t), st()) == 0
    assert L().mvg_merge_sp(p(out.t), p(merged.t), 0, 1.0, st()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.intact("sp").float()).all()) and bool(torch.isnan(merged.intact("merged")).all())
    assert int(word.intact("word").item()) == 0
    print("PREP-FORMS n=0 split_f32 split_f32_ranged merge_sp: returned 0, outputs untouched")


# ---------------------------------------------------------------- B. the batched weight prep
class PrepLaunch:
    """The records of one mode in ONE mvg_weights_prep_batch launch, in `order`: sources, guarded destinations, cleared stat pairs."""

    def __init__(self, mode, order, blocks_per_item):
        from rot_mvgaze_amd import ops
        recs = R.MODE1_RECORDS if mode == 1 else R.MODE0_RECORDS
        self.mode, self.recs = mode, recs
        self.w = [R.record_weights(mode, i).to(dev()) for i in range(len(recs))]
        self.wk, self.wt = [], []
        for name, cout, rs, cin, cin_pad, has_t, mag in recs:
            if mode == 1:
                self.wk.append(Guarded((cout, rs * cin // 8, 2, 8), torch.float16))
                self.wt.append(Guarded((cin, rs * cout // 8, 2, 8), torch.float16) if has_t else None)
            else:
                self.wk.append(Guarded((cout, rs, cin_pad), torch.bfloat16))
                self.wt.append(Guarded((cin_pad, rs, cout), torch.bfloat16) if has_t else None)
        self.stat = Guarded((len(recs), 2), init=0.0)                     # cleared, as Backbone._prepare_weights does
        rows = []
        for i in order:
            name, cout, rs, cin, cin_pad, has_t, mag = recs[i]
            rows.append([self.w[i].data_ptr(), self.wk[i].t.data_ptr(), self.wt[i].t.data_ptr() if has_t else 0, cout | (rs << 32),
                         cin | (cin_pad << 32), self.stat.t[i].data_ptr()])
        self.table = torch.tensor(rows, dtype=torch.int64).to(dev())
        ops.weights_prep_batch(self.table, len(order), mode, blocks_per_item)

    def outputs(self):
        out = [self.stat.t.view(torch.int32)]
        for k, t in zip(self.wk, self.wt):
            out += [k.t.view(torch.int16)] + ([t.t.view(torch.int16)] if t else [])
        return out


def check_prep(launch, what):
    recs = launch.recs
    stat = bits32(launch.stat.intact(what + " stat")).reshape(len(recs), 2)
    for i, rec in enumerate(recs):
        name = f"{what} {rec[0]}"
        w = R.record_weights(launch.mode, i)
        if launch.mode == 1:
            bits0, sinv, scale, krsc, crsk = R.mode1_expected(w)
            print(f"PREP-FORMS {name} {R.mode1_branch(rec)}: stat {stat[i, 0]:#010x} {stat[i, 1]:#010x} (host {bits0:#010x} "
                  f"{int(sinv.view(np.uint32)):#010x}, scale 2^{int(np.log2(scale))})")
            assert stat[i, 0] == bits0 and stat[i, 1] == sinv.view(np.uint32), f"{name}: the stat pair is not {{max |w| bits, 2^-k}}"
            held_sp(launch.wk[i], krsc, name + " KRSC")
            if launch.wt[i]:
                held_sp(launch.wt[i], crsk, name + " CRSK " + R.mode1_branch(rec))
            if rec[6] == 0.0:
                assert stat[i, 0] == 0 and stat[i, 1] == np.float32(1.0).view(np.uint32) and not u16(launch.wk[i].t).any()
        else:
            wk, wt = R.mode0_expected(w, rec[4])
            assert int(stat[i, 0]) == 0 and int(stat[i, 1]) == 0, f"{name}: mode 0 wrote a stat pair"
            for got, want, nm in ((launch.wk[i], wk, "KRSC"), (launch.wt[i], wt, "CRSK")):
                if got is None:
                    continue
                differ = int((u16(got.intact(name + " " + nm)) != u16(want)).sum())
                print(f"PREP-FORMS {name} {nm} {R.mode0_branch(rec)}: elements differing from w.to(bfloat16) {differ} of {want.numel()}")
                assert differ == 0, f"{name} {nm}"
            if rec[3] != rec[4]:
                assert not u16(launch.wk[i].t).reshape(rec[1], rec[2], rec[4])[..., rec[3]:].any(), "padding channels must be zero"


@pytest.mark.parametrize("blocks_per_item", R.BLOCKS_PER_ITEM)
@pytest.mark.parametrize("mode", [1, 0])
def test_prep_forms_weights_prep_batch(mode, blocks_per_item):
    n = len(R.MODE1_RECORDS if mode == 1 else R.MODE0_RECORDS)
    what = f"prep mode={mode} blocks={blocks_per_item}"
    fwd = PrepLaunch(mode, list(range(n)), blocks_per_item)
    check_prep(fwd, what)
    rev = PrepLaunch(mode, list(range(n))[::-1], blocks_per_item)
    check_prep(rev, what + " reversed")
    for a, b in zip(fwd.outputs(), rev.outputs()):
        assert torch.equal(a, b), what + ": a record's bits depend on its place in the table"


def rec_desc(rec):
    from rot_mvgaze_amd._lib import ConvDesc
    name, cout, rs, cin, cin_pad, has_t, mag = rec
    r, s = {1: (1, 1), 9: (3, 3), 49: (7, 7), 7: (7, 1)}[rs]
    return ConvDesc(1, 1, r, s, cin_pad, cout, r, s, 1, 0, 1, 1)


def test_prep_forms_single_record_forms_give_the_batched_bits():
    from rot_mvgaze_amd import ops
    one = PrepLaunch(1, list(range(len(R.MODE1_RECORDS))), 0)
    for i, rec in enumerate(R.MODE1_RECORDS):
        wk, wt = ops.split_weights(rec_desc(rec), one.w[i].view(rec[1], rec[2], rec[3]), rec[5])
        same = torch.equal(wk.view(torch.int16).view(-1), one.wk[i].t.view(torch.int16).view(-1))
        same_t = wt is None or torch.equal(wt.view(torch.int16).view(-1), one.wt[i].t.view(torch.int16).view(-1))
        same_s = torch.equal(wk.sinv.view(torch.int32), one.stat.t[i, 1:2].view(torch.int32))
        print(f"PREP-FORMS prep mode=1 {rec[0]} split_weights: KRSC {same} CRSK {same_t} 2^-k {same_s}")
        assert same and same_t and same_s, rec[0]
    zero = PrepLaunch(0, list(range(len(R.MODE0_RECORDS))), 0)
    for i, rec in enumerate(R.MODE0_RECORDS):
        wk, wt = ops.cast_weights_bf16(rec_desc(rec), zero.w[i], rec[3], rec[5])
        same = torch.equal(wk.view(torch.int16).view(-1), zero.wk[i].t.view(torch.int16).view(-1))
        same_t = wt is None or torch.equal(wt.view(torch.int16).view(-1), zero.wt[i].t.view(torch.int16).view(-1))
        print(f"PREP-FORMS prep mode=0 {rec[0]} cast_weights_bf16: KRSC {same} CRSK {same_t}")
        assert same and same_t, rec[0]


def test_prep_forms_weights_prep_batch_rejections():
    from rot_mvgaze_amd import ops
    w = torch.ones(64, 1, 64, device=dev())
    wk, stat = Guarded((64, 8, 2, 8), torch.float16), Guarded((1, 2), init=0.0)
    table = torch.tensor([[w.data_ptr(), wk.t.data_ptr(), 0, 64 | (1 << 32), 64 | (64 << 32), stat.t.data_ptr()]], dtype=torch.int64).to(dev())
    for n, mode, blocks in ((0, 1, 0), (1, 2, 0), (1, 1, 4097), (1, 0, -1)):
        assert L().mvg_weights_prep_batch(C.c_void_p(table.data_ptr()), n, mode, blocks, st()) != 0
        assert b"weights_prep_batch: bad arguments" in L().mvg_last_error()
    with pytest.raises(RuntimeError, match="bad arguments"):
        ops.weights_prep_batch(table, 1, 2, 0)
    torch.cuda.synchronize()
    assert bool(torch.isnan(wk.intact("wk").float()).all()) and not bits32(stat.intact("stat")).any(), "a rejected call launched"
    print("PREP-FORMS prep rejections n=0 mode=2 blocks=4097 blocks=-1: refused, nothing launched")


# ---------------------------------------------------------------- C. the row-window builders
def offset_view(x):
    """x on the device as a view that starts 8 bytes - not 16 - into its allocation."""
    buf = torch.empty(x.numel() + 2, dtype=torch.float32, device=dev())
    v = buf[2:].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 == 8
    return v


@pytest.mark.parametrize("size", R.ROWWINDOW_SPLIT_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_prep_forms_rowwindow_split_from_nhwc4_and_nchw(size):
    n, h, w = size
    what = f"rowwindow {n}x{h}x{w}"
    x = R.image(n, h, w)
    want = R.rowwindow_split_ref(x.transpose(0, 2, 3, 1)).reshape(n, h, w // 2, 32)
    x4 = np.zeros((n, h, w, 4), dtype=np.float32)
    x4[..., :3] = x.transpose(0, 2, 3, 1)
    x4d, xcd = torch.from_numpy(x4).to(dev()), offset_view(torch.from_numpy(x))
    a = Guarded((n, h, w // 2, 4, 2, 8), torch.float16)
    call(L().mvg_stem_rowwindow_split(p(x4d), p(a.t), n, h, w, st()), "stem_rowwindow_split")
    held_sp(a, want, what + " split")
    b = Guarded((n, h, w // 2, 4, 2, 8), torch.float16)
    call(L().mvg_stem_rowwindow_split_nchw(p(xcd), p(b.t), n, h, w, st()), "stem_rowwindow_split_nchw")
    same = torch.equal(b.intact(what + " split_nchw").view(torch.int16), a.t.view(torch.int16))
    print(f"PREP-FORMS {what} split_nchw: bit-equal to the NHWC4 form {same}")
    assert same
    del a, b, x4d, xcd
    free()


@pytest.mark.parametrize("size", R.ROWWINDOW_BF16_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_prep_forms_rowwindow_bf16(size):
    n, h, w = size
    what = f"rowwindow {n}x{h}x{w} bf16"
    x = R.image(n, h, w, seed=1)
    want = torch.from_numpy(R.rowwindow_bf16_ref(x.transpose(0, 2, 3, 1)).reshape(n, h, w // 4, 64)).to(torch.bfloat16)
    xcd = offset_view(torch.from_numpy(x))
    a = Guarded((n, h, w // 4, 64), torch.bfloat16)
    call(L().mvg_stem_rowwindow_bf16(p(xcd), p(a.t), n, h, w, st()), "stem_rowwindow_bf16")
    differ = int((a.intact(what).view(torch.int16) != want.view(torch.int16).to(dev())).sum())
    print(f"PREP-FORMS {what}: elements differing from the gather rounded to bf16 {differ} of {want.numel()}")
    assert differ == 0
    del a, xcd
    free()


# ---------------------------------------------------------------- D. the stems' conv forms
def stem_desc(case, cin):
    from rot_mvgaze_amd._lib import ConvDesc
    G, N, H, W, cout = case
    return ConvDesc.make(G, N, H, W, cin, cout, 7, 2, 3)


def cid(case):
    return "x".join(map(str, case))


def held_f32(out, ref, what, e32=None, split=False):
    """An fp32 output against float64: finite everywhere, per element, and for the split kernels (`split`) SPLIT_VS_F64 and - where
    the fp32-MFMA kernel serves the shape: e32, its error on the same inputs - SPLIT_VS_FP32_KERNEL."""
    got = out.intact(what) if isinstance(out, Guarded) else out
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values (an unwritten output, or an unwritten slab summed into it)"
    e = rel_l2(got.cpu(), ref)
    worst = (got.cpu().double() - ref).abs().max().item() / (ref.abs().max().item() + 1e-30)
    print(f"PREP-FORMS {what}: rel-L2 {e:.3e}" + (f" (fp32-MFMA {e32:.3e})" if e32 is not None else "") + f", largest element error {worst:.3e} of max |ref|")
    if split:
        assert e <= SPLIT_VS_F64, f"{what}: split {e:.2e} against float64"
    if e32 is not None:
        assert e <= SPLIT_VS_FP32_KERNEL * e32 + 1e-7, f"{what}: split {e:.2e}, fp32-MFMA kernel {e32:.2e}"
    close(got, ref, 2e-5, what)


def split_partials(stats, y_ref, rows, what):
    """Every statistics partial of the split stem against float64 over exactly the 64 rows it covers; later ones are never read."""
    G, P = stats.shape[0], stats.shape[1]
    yg = y_ref.reshape(G, rows, -1)
    covered = -(-rows // 64)
    assert covered <= P
    st_ = stats[:, :covered].cpu().double()
    assert bool(torch.isfinite(st_).all()), f"{what}: a partial with rows was not written"
    worst = [0.0, 0.0]
    for pi in range(covered):
        blk = yg[:, 64 * pi:min(64 * pi + 64, rows)]
        s, q = R.partial_stats(blk)
        tol_s = 1e-4 * s.abs() + 1e-4 * float(blk.abs().sum(1).max())
        tol_q = 1e-3 * q.abs() + 1e-5 * float(q.max()) + 1e-12
        worst[0] = max(worst[0], float(((st_[:, pi, 0] - s).abs() / tol_s).max()))
        worst[1] = max(worst[1], float(((st_[:, pi, 1] - q).abs() / tol_q).max()))
    print(f"PREP-FORMS {what} partials: {covered} of {P} hold rows; sum at {worst[0]:.3e} of its bar, centred squares at {worst[1]:.3e}")
    assert max(worst) <= 1.0, f"{what}: a partial's sum / centred sum of squares is at {worst} of its bar"
    return covered


@pytest.mark.parametrize("case,fwd,wg", R.SPLIT_STEM_CASES, ids=[cid(c) for c, _, _ in R.SPLIT_STEM_CASES])
def test_prep_forms_split_stem(case, fwd, wg):
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import ConvDesc
    G, N, H, W, cout = case
    d = stem_desc(case, 4)
    ho, wo = d.ho, d.wo
    rows = N * ho * wo
    pb = R.split_stem_problem(case)
    x = pb.x.to(dev())
    xw = ops.stem_rowwindow_split(x)
    w8 = R.stem_taps_rowwindow(pb.w)
    scale = R.sp_scale_for(float(w8.abs().max()))
    wk = ops.split_f32(w8.view(cout, 224).to(dev()), scale)               # the KRSC sp copy of [cout][7][1][32] with its 2^-k
    w4 = torch.zeros(cout, 7, 7, 4)
    w4[..., :3] = pb.w
    w4 = w4.to(dev())
    # (the fp32-MFMA kernel takes power-of-two channel counts under a 7x7 filter: at cout = 96 the float64 bars stand alone)
    mfma = cout & (cout - 1) == 0
    e32 = None
    if mfma:
        y32 = torch.empty(G, N, ho, wo, cout, device=dev())
        ops.conv_fprop(d, x, w4, y32, None, False, None)
        e32 = rel_l2(y32.cpu(), pb.y_ref)
        del y32
    P, rpp = ops.conv_stats_partials_split(ConvDesc.make(G, N, ho, wo, 32, cout, 1, 1, 0))
    assert rpp == 64
    got, planned = [], []
    for (name, res, _), form in zip(settings(), fwd):
        with reserved_cus(res):
            plan = ops.stem_plan_query_split(d)
            assert plan["fwd"] == form, f"{cid(case)} {name}: the forward moved to {plan['fwd']}"
            assert plan["wgrad"] == wg, f"{cid(case)} {name}: the weight gradient moved to {plan['wgrad']}"
            _seen.add(("split_fwd",) + form)
            _seen.add(("split_wgrad",) + wg)
            planned.append(L().mvg_stem_wgrad_splits_split(C.byref(d)))
            y, stats = Guarded((G, N, ho, wo, cout)), Guarded((G, P, 2, cout))
            ops.stem_fprop_split(d, xw, wk, y.t, stats.t)
        what = f"{cid(case)} split_fwd {form[0]}x{form[1]} stages={form[2]} ({name})"
        held_f32(y, pb.y_ref, what + " y", e32, split=True)
        covered = split_partials(stats.intact(what + " stats"), pb.y_ref, rows, what)
        got.append((y.t, stats.t[:, :covered].clone()))
        y2 = Guarded((G, N, ho, wo, cout))
        with reserved_cus(res):
            ops.stem_fprop_split(d, xw, wk, y2.t, None)
        assert torch.equal(y2.intact(what + " without statistics"), y.t), "the statistics must not change y"
        del y2
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]), f"{cid(case)}: y / partials differ across the CU settings"
    if case == R.SPLIT_STEM_BIG:
        del got, y, stats, xw
        free()
        return
    # weight gradient with caller-chosen slab counts, fresh and accumulating onto ones
    assert min(planned) >= 1
    gscale = 2.0 ** float(torch.floor(torch.log2(2.0 ** 14 / pb.gy.abs().max())))
    gyd = pb.gy.to(dev())
    gys = ops.split_f32(gyd, gscale)
    e32 = None
    if mfma:
        dw32 = torch.empty(cout, 7, 7, 4, device=dev())
        ops.conv_wgrad(d, x, gyd, dw32, False)
        e32 = rel_l2(dw32[..., :3].cpu(), pb.dw_ref)
    name = "%dx%d%s" % (wg[0], wg[1], "incr" if wg[2] else "decode")
    for splits in R.wgrad_split_counts(G * rows, 16, planned):
        for accumulate in (False, True):
            dw = Guarded((cout, 7, 8, 4), init=1.0 if accumulate else None)
            ws = Guarded((splits * cout * 224,)) if splits > 1 else None
            call(L().mvg_stem_wgrad_split(C.byref(d), p(xw), p(gys), p(gys.sinv), p(dw.t), p(ws.t if ws else None), splits, int(accumulate), st()),
                 "stem_wgrad_split")
            if ws:
                ws.intact("slabs")
            what = f"{cid(case)} split_wgrad {name} splits={splits} accumulate={accumulate}"
            assert bool(torch.isfinite(dw.intact(what)).all()), f"{what}: non-finite values (an unwritten slab)"
            # (the padding taps j = 0 and c = 3 see real pixels / zeros: the caller drops them)
            held_f32(dw.t[:, :, 1:, :3], pb.dw_ref + (1.0 if accumulate else 0.0), what, None if accumulate else e32, split=not accumulate)


def fold_partials(stats, y_ref, G, rows_f, cout, what):
    """Partial 2 pi + par of channel c = the output pixels (n, oy, 2 m + par) of folded rows 64 pi .. 64 pi + 63."""
    st_ = stats.cpu().double()                                  # [G, 2P, 2, cout]
    assert bool(torch.isfinite(st_).all()), f"{what}: a partial was not written"
    yf = y_ref.reshape(G, rows_f, 2, cout)
    P = st_.shape[1] // 2
    worst = [0.0, 0.0]
    for pi in range(P):
        for par in range(2):
            blk = yf[:, 64 * pi:64 * pi + 64, par]
            if blk.shape[1] == 0:
                assert bool((st_[:, 2 * pi + par] == 0).all()), f"{what}: partial {2 * pi + par} holds no rows: it must be exactly (0, 0)"
                continue
            for k, want in enumerate(R.partial_stats(blk)):
                for g in range(G):
                    err = (st_[g, 2 * pi + par, k] - want[g]).abs().max().item() / (want[g].abs().max().item() + 1e-300)
                    worst[k] = max(worst[k], err)
    print(f"PREP-FORMS {what} folded partials: sum {worst[0]:.3e} centred squares {worst[1]:.3e} (of the partial's largest)")
    assert max(worst) <= 2e-4, f"{what}: a folded partial's sum / centred sum of squares: {worst}"


@pytest.mark.parametrize("case,fwd,wg", R.BF16_STEM_CASES, ids=[cid(c) for c, _, _ in R.BF16_STEM_CASES])
def test_prep_forms_bf16_folded_stem(case, fwd, wg):
    from rot_mvgaze_amd import ops
    from rot_mvgaze_amd._lib import ConvDesc
    G, N, H, W, cout = case
    d = stem_desc(case, 8)
    ho, wo = d.ho, d.wo
    rows_f = N * ho * (wo // 2)
    plan = ops.stem_plan_query_bf16(d)
    assert (plan["fwd"]["kernel"], plan["fwd"]["bn"]) == fwd, f"{cid(case)}: the forward moved to {plan['fwd']}"
    assert plan["wgrad"] == wg, f"{cid(case)}: the weight gradient moved to {plan['wgrad']}"
    _seen.add(("bf16_fwd",) + fwd)
    _seen.add(("bf16_wgrad",) + wg)
    pb = R.bf16_stem_problem(case)
    xd = pb.x.to(dev())
    xw = torch.empty(G * N, H, W // 4, 64, dtype=torch.bfloat16, device=dev())
    ops.stem_rowwindow_bf16(xd, xw)
    wf = R.stem_taps_folded(pb.w.permute(0, 2, 3, 1)).to(torch.bfloat16).to(dev())
    P, rpp = ops.conv_stats_partials(ConvDesc.make(G, N, ho, wo // 2, 64, 2 * cout, 1, 1, 0), True)
    assert (P, rpp) == (2 * -(-rows_f // 128), 64)
    what = f"{cid(case)} bf16_fwd {fwd[0]}{fwd[1]}"
    y, stats = Guarded((G, N, ho, wo, cout), torch.bfloat16), Guarded((G, 2 * P, 2, cout))
    ops.stem_fprop_bf16(d, xw, wf, y.t, stats.t)
    got = y.intact(what + " y")
    assert bool(torch.isfinite(got.float()).all()), f"{what}: non-finite values (an element the launch did not write)"
    ratio = B.bound_ratio(got, pb.y_ref, pb.magnitude)
    print(f"PREP-FORMS {what} y: largest bound ratio {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: an element is at {ratio:.3f} of its bound 2^-8 |ref| + 1.004 * 2e-5 * {pb.magnitude:.3e}"
    fold_partials(stats.intact(what + " stats"), pb.y_ref, G, rows_f, cout, what)
    y2 = Guarded((G, N, ho, wo, cout), torch.bfloat16)
    ops.stem_fprop_bf16(d, xw, wf, y2.t, None)
    assert torch.equal(y2.intact("y without statistics"), y.t), "the statistics must not change y"
    # every output pixel counted exactly once: x = 1, the centre tap of channel 0 = 1 -> y = 1 at every pixel, so a partial's
    # sum is its pixel count (exact in fp32) and bn_finalize's mean is total count / rows
    ones = torch.ones(G * N, 3, H, W, device=dev())
    xw1 = torch.empty_like(xw)
    ops.stem_rowwindow_bf16(ones, xw1)
    wc = torch.zeros(cout, 7, 7, 3)
    wc[:, 3, 3, 0] = 1.0
    y1, stats1 = Guarded((G, N, ho, wo, cout), torch.bfloat16), Guarded((G, 2 * P, 2, cout))
    ops.stem_fprop_bf16(d, xw1, R.stem_taps_folded(wc).to(torch.bfloat16).to(dev()), y1.t, stats1.t)
    assert bool((y1.intact("y of ones").float() == 1.0).all())
    s1 = stats1.intact("stats of ones").cpu()
    full = rows_f // 64
    counts_ok = bool((s1[:, :2 * full, 0] == 64.0).all()) and bool((s1[:, 2 * full:] == 0.0).all()) and bool((s1[:, :, 1] == 0.0).all())
    mean, invstd, sc, sh = (Guarded((G, cout)) for _ in range(4))
    one, zero = torch.ones(cout, device=dev()), torch.zeros(cout, device=dev())
    ops.bn_finalize(stats1.t, G, 2 * P, rpp, N * ho * wo, cout, one, zero, zero.clone(), one.clone(), 0.1, 1e-5, mean.t, invstd.t, sc.t, sh.t)
    mean_ok = bool((mean.intact("mean") == 1.0).all())
    print(f"PREP-FORMS {what} pixel counts: every partial with rows counts 64 {counts_ok}, total {int(s1[0, :, 0, 0].sum())} of {N * ho * wo}, "
          f"bn_finalize's mean of an all-ones y is exactly 1 {mean_ok}")
    assert counts_ok and mean_ok and int(s1[0, :, 0, 0].sum()) == N * ho * wo
    # weight gradient with caller-chosen slab counts
    planned = [0, 0]
    for i, (name, res, _) in enumerate(settings()):
        with reserved_cus(res):
            planned[i] = L().mvg_stem_wgrad_splits_bf16(C.byref(d))
    assert min(planned) >= 1
    gyd = pb.gy.to(torch.bfloat16).to(dev())
    name = "%dx%d%s" % (wg[0], wg[1], "incr" if wg[2] else "decode")
    for splits in R.wgrad_split_counts(G * rows_f, 64, planned):
        for accumulate in (False, True):
            dw = Guarded((2 * cout, 7, 16, 4), init=1.0 if accumulate else None)
            ws = Guarded((splits * 2 * cout * 448,)) if splits > 1 else None
            call(L().mvg_stem_wgrad_bf16(C.byref(d), p(xw), p(gyd), p(dw.t), p(ws.t if ws else None), splits, int(accumulate), st()), "stem_wgrad_bf16")
            if ws:
                ws.intact("slabs")
            what = f"{cid(case)} bf16_wgrad {name} splits={splits} accumulate={accumulate}"
            assert bool(torch.isfinite(dw.intact(what)).all()), f"{what}: non-finite values (an unwritten slab)"
            held_f32(R.unfold_dw(dw.t), pb.dw_ref + (2.0 if accumulate else 0.0), what)


def test_prep_forms_stem_rejections():
    from rot_mvgaze_amd import ops
    xw = torch.zeros(4096, dtype=torch.float16, device=dev())
    y = Guarded((4096,))
    for case, cin, fn, msg in (((1, 2, 16, 15, 64), 4, "split", "even width"), ((1, 2, 16, 16, 48), 4, "split", "multiple of 32"),
                               ((1, 1, 8, 8, 64), 8, "bf16", "multiple of 64"), ((1, 4, 16, 6, 64), 8, "bf16", "width")):
        d = stem_desc(case, cin)
        with pytest.raises(RuntimeError, match=msg):
            if fn == "split":
                ops.stem_fprop_split(d, xw, xw, y.t, None)
            else:
                ops.stem_fprop_bf16(d, xw.view(torch.bfloat16), xw.view(torch.bfloat16), y.t.view(torch.bfloat16), None)
        with pytest.raises(RuntimeError, match=msg):
            (ops.stem_plan_query_split if fn == "split" else ops.stem_plan_query_bf16)(d)
        rc = (L().mvg_stem_wgrad_split(C.byref(d), p(xw), p(xw), None, p(y.t), None, 1, 0, st()) if fn == "split" else
              L().mvg_stem_wgrad_bf16(C.byref(d), p(xw), p(xw), p(y.t), None, 1, 0, st()))
        assert rc != 0 and msg.encode() in L().mvg_last_error()
        print(f"PREP-FORMS {cid(case)} {fn} stem: refused ({msg})")
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.intact("y")).all()), "a rejected call launched"


def test_prep_forms_union_of_guarded_forms_and_exception_count():
    """Runs last: what the guards above recorded is the whole table; and the tally of the sp exception."""
    total = sum(_subnormal_differences)
    print(f"PREP-FORMS forms seen: {sorted(_seen, key=str)}")
    print(f"PREP-FORMS subnormal-piece elements that differed, over {len(_subnormal_differences)} sp comparisons: {total}"
          + (" (the device rounds fp16 subnormals as numpy does)" if total == 0 else " (the device's conversion differs on subnormal pieces)"))
    assert _seen == R.FORMS, f"never run: {sorted(R.FORMS - _seen, key=str)}; not in the table: {sorted(_seen - R.FORMS, key=str)}"
