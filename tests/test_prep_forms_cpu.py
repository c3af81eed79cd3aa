"""The host references and case tables of tests/prep_forms_ref.py checked on their own (no GPU): the sp reference round-trips
as csrc/elem.h states, sp_scale_for behaves as elem.h's, every weight-prep record takes the branch it is in the table for and
the tables reach every branch, the row-window gathers are the comments' index rules, and the stems' host-only plan queries
(mvg_stem_plan_query_split / _bf16) are declared, bound, launch nothing and agree with the launch rules restated in the tables."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import rot_mvgaze_amd  # noqa: F401
import prep_forms_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAGNITUDES = (1.0, 1e-3, 300.0, 0.08)


def scaled_gaussian(mag, n=1 << 18, seed=0):
    w = (np.random.default_rng(seed).standard_normal(n) * mag).astype(np.float32)
    scale = R.sp_scale_for(np.abs(w).max())
    return w, scale


@pytest.mark.parametrize("mag", MAGNITUDES)
def test_sp_reference_round_trips_within_the_format_bound(mag):
    w, scale = scaled_gaussian(mag)
    stored = w * np.float32(scale)
    pieces = R.sp_pieces(stored)
    assert pieces.shape == (w.size // 8, 2, 8) and pieces.dtype == np.uint16
    back = R.sp_merge(pieces, 1.0 / scale).astype(np.float64)
    v = w.astype(np.float64)
    assert bool((np.abs(back - v) <= R.SP_ULP * np.abs(v) + R.SP_FLOOR / scale).all())
    exact = float((back == v).mean())
    print(f"PREP-FORMS cpu magnitude {mag}: exact round trips {exact:.4f}")
    assert 0.72 <= exact <= 0.78, "three values in four come back exactly (conv_split.hip's header)"
    # the exception of the GPU tests is rare at the table's magnitudes and sits on small stored values only
    sub = R.subnormal_piece(pieces)
    share = float(sub.mean())
    print(f"PREP-FORMS cpu magnitude {mag}: subnormal second pieces {share:.5%}")
    assert share <= 5e-4
    assert not sub.any() or float(np.abs(stored[sub]).max()) < 512.0
    # the reference against itself: nothing differs.  A second piece that differs in its last place where it is subnormal is
    # counted under the exception and is within the bound when it is the neighbouring value on the other side of v (2^-24 apart,
    # the nearer one at most 2^-25 away: only a tie can go either way); a piece flushed to zero is counted too but misses the
    # bound by orders of magnitude - the bound admits another rounding of the last place, not the loss of the piece
    assert R.sp_compare(pieces, stored) == (0, 0, 0.0)
    flushed = pieces.copy()
    h2 = flushed[:, 1, :]
    h2[((h2 & 0x7C00) == 0)] &= 0x8000
    wrong, excused, worst = R.sp_compare(flushed, stored)
    assert wrong == 0 and excused == int(sub.sum())
    assert worst > 1.0 or excused == 0
    broken = pieces.copy()
    broken[3, 0, 5] ^= 1                                     # one bit of one first piece
    assert R.sp_compare(broken, stored)[0] == 1


def test_sp_pieces_layout_and_corner_values():
    v = np.arange(48, dtype=np.float32).reshape(2, 24) + np.float32(0.001)
    p = R.sp_pieces(v)
    flat = p.reshape(-1)
    for row in range(2):
        for c in range(24):
            h1 = np.float16(v[row, c])
            h2 = np.float16(v[row, c] - np.float32(h1))
            for piece, h in ((0, h1), (1, h2)):
                assert flat[((row * 3 + c // 8) * 2 + piece) * 8 + c % 8] == h.view(np.uint16)
    big = R.sp_pieces(np.array([70000.0, -70000.0, 65504.0, 65519.9, 65520.0, 0.0, -0.0, 1.0], dtype=np.float32))
    assert list(big[0, 0, :5]) == [0x7C00, 0xFC00, 0x7BFF, 0x7BFF, 0x7C00] and big[0, 0, 6] == 0x8000
    assert R.range_word(np.array([65520.0], dtype=np.float32)) == R.RANGE_OVER_BITS
    assert R.range_word(np.array([-3.0, 2.0], dtype=np.float32)) == 0x40400000


def test_sp_scale_for_matches_elem_h():
    for mag in (1e-25, 1e-9, 1e-3, 0.08, 1.0, 300.0, 65504.0, 1e6, 1e30):
        for f in (1.0, 1.37, 1.999):
            s = R.sp_scale_for(mag * f)
            assert 2.0 ** 14 <= float(np.float32(mag * f)) * s < 2.0 ** 15 and np.log2(s) == round(np.log2(s))
    assert R.sp_scale_for(2.0 ** 14) == 1.0 and R.sp_scale_for(np.nextafter(np.float32(2.0 ** 14), np.float32(0))) == 2.0
    assert R.sp_scale_for(1e-38) == 2.0 ** 100 and R.sp_scale_for(2.0 ** 120) == 2.0 ** -100        # the clamp
    for degenerate in (0.0, -1.0, float("nan"), 3.0e38, float("inf")):
        assert R.sp_scale_for(degenerate) == 1.0
    # the source says the same: the constants of elem.h's function
    src = open(os.path.join(ROOT, "rot-mvgaze_amd", "csrc", "elem.h")).read()
    body = src[src.index("float sp_scale_for(float bound)"):]
    body = body[:body.index("}") + 1]
    assert "3.0e38f" in body and "15 - e" in body and "k > 100 ? 100 : (k < -100 ? -100 : k)" in body


def test_every_record_takes_the_branch_it_is_there_for():
    want1 = {"3x3_64to128": "gather", "1x1_96to160": "gather", "1x1_256to320": "tiled", "1x1_64to64": "tiled",
             "1x1_128to64_no_wt": "none", "stem_64x7x1x32": "none", "zeros_3x3_32to32": "gather"}
    want0 = {"1x1_256to320": "linear", "1x1_256to320_no_wt": "linear", "3x3_64to128": "element", "7x7_3to64_pad8": "element",
             "stem_fold_128x7x1x64": "element", "1x1_96to160": "element"}
    assert {r[0]: R.mode1_branch(r) for r in R.MODE1_RECORDS} == want1
    assert {r[0]: R.mode0_branch(r) for r in R.MODE0_RECORDS} == want0
    # the predicates are the kernel's: its two conditions, as written in the source
    src = open(os.path.join(ROOT, "rot-mvgaze_amd", "csrc", "conv_split.hip")).read()
    assert "const bool tiled = wt != nullptr && rs == 1 && (cin % 64) == 0 && (cout % 64) == 0;" in src
    assert "if (rs == 1 && cin == cin_pad && (cin % 64) == 0 && (cout % 64) == 0) {" in src


def test_the_tables_reach_every_branch_in_both_modes():
    assert {R.mode1_branch(r) for r in R.MODE1_RECORDS} == {"gather", "tiled", "none"}
    assert {R.mode0_branch(r) for r in R.MODE0_RECORDS} == {"linear", "element"}
    assert any(R.mode0_branch(r) == "linear" and r[5] for r in R.MODE0_RECORDS)
    assert any(R.mode0_branch(r) == "linear" and not r[5] for r in R.MODE0_RECORDS)
    assert any(r[3] != r[4] for r in R.MODE0_RECORDS), "a record with channel padding"
    t = [R.tiles(r) for r in R.MODE1_RECORDS if R.mode1_branch(r) == "tiled"]
    assert 1 in t and any(16 < n < 64 for n in t), "one tile; more tiles than 16 workgroups and fewer than 64"
    mags = [r[6] for r in R.MODE1_RECORDS if r[6] > 0]
    assert min(mags) <= 1e-3 and max(mags) >= 300 and 0.0 in [r[6] for r in R.MODE1_RECORDS]
    for mode, recs in ((1, R.MODE1_RECORDS), (0, R.MODE0_RECORDS)):
        for i, r in enumerate(recs):
            w = R.record_weights(mode, i)
            assert tuple(w.shape) == (r[1], r[2], r[3]) and (mode == 0 or r[3] % 8 == 0)
    stem = R.record_weights(1, 5).view(64, 7, 8, 4)
    assert not stem[:, :, 0].any() and not stem[..., 3].any() and stem[:, :, 1:, :3].abs().min() > 0
    fold = R.record_weights(0, 4).view(128, 7, 16, 4)
    assert torch.equal(fold[:64, :, 1:8], fold[64:, :, 3:10]) and not fold[:64, :, 8:].any() and not fold[64:, :, :3].any()
    zero = R.mode1_expected(R.record_weights(1, 6))
    assert zero[0] == 0 and zero[1] == 1.0 and not zero[3].any()
    k = R.mode1_expected(R.record_weights(1, 2))
    assert 2.0 ** 14 <= np.abs(k[3]).max() < 2.0 ** 15 and np.array_equal(k[4], k[3].T)         # 1x1: CRSK is the transpose


def test_rowwindow_gathers_are_the_index_rules():
    x = R.image(2, 3, 8, seed=1).transpose(0, 2, 3, 1)                  # NHWC3
    s = R.rowwindow_split_ref(x)
    b = R.rowwindow_bf16_ref(x)
    for ox in range(4):
        for j in range(8):
            col = 2 * ox - 4 + j
            want = x[:, :, col] if 0 <= col < 8 else 0.0
            assert np.array_equal(s[:, :, ox, j, :3], np.broadcast_to(want, (2, 3, 3))) and not s[:, :, ox, j, 3].any()
    for m in range(2):
        for j in range(16):
            col = 4 * m - 4 + j
            want = x[:, :, col] if 0 <= col < 8 else 0.0
            assert np.array_equal(b[:, :, m, j, :3], np.broadcast_to(want, (2, 3, 3))) and not b[:, :, m, j, 3].any()
    for n, h, w in R.ROWWINDOW_SPLIT_SIZES:
        assert w % 2 == 0
    for n, h, w in R.ROWWINDOW_BF16_SIZES:
        assert w % 4 == 0
    assert R.ROWWINDOW_SPLIT_SIZES[-1][0] * R.ROWWINDOW_SPLIT_SIZES[-1][1] * R.ROWWINDOW_SPLIT_SIZES[-1][2] > 2097152
    assert R.ROWWINDOW_BF16_SIZES[-1][0] * R.ROWWINDOW_BF16_SIZES[-1][1] * R.ROWWINDOW_BF16_SIZES[-1][2] > 2097152
    assert any(h == 1 for _, h, _ in R.ROWWINDOW_SPLIT_SIZES) and any(w == 2 for _, _, w in R.ROWWINDOW_SPLIT_SIZES)
    assert any(h == 1 for _, h, _ in R.ROWWINDOW_BF16_SIZES) and any(w == 4 for _, _, w in R.ROWWINDOW_BF16_SIZES)
    assert R.SPLIT_SIZES[-1] // 8 > 8192 * 256


def stem_desc(case, cin):
    from rot_mvgaze_amd._lib import ConvDesc
    G, N, H, W, cout = case
    return ConvDesc.make(G, N, H, W, cin, cout, 7, 2, 3)


def test_stem_plan_queries_declared_bound_and_launching_nothing():
    from rot_mvgaze_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "rotmvgaze.h")).read()
    for name, nargs in (("mvg_stem_plan_query_split", 7), ("mvg_stem_plan_query_bf16", 5)):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert len(_lib.SIGNATURES[name][1]) == nargs
    L = _lib.lib()
    ok = stem_desc((1, 2, 16, 16, 64), 4)
    assert L.mvg_stem_plan_query_split(ok, None, None, None, None, None, None) == 0            # every out-pointer may be NULL
    okb = stem_desc((1, 4, 16, 16, 64), 8)
    assert L.mvg_stem_plan_query_bf16(okb, None, None, None, None) == 0
    assert L.mvg_stem_plan_query_split(None, None, None, None, None, None, None) == -1
    assert L.mvg_stem_plan_query_bf16(None, None, None, None, None) == -1
    with pytest.raises(RuntimeError, match="even width"):
        ops.stem_plan_query_split(stem_desc((1, 2, 16, 15, 64), 4))
    with pytest.raises(RuntimeError, match="multiple of 32"):
        ops.stem_plan_query_split(stem_desc((1, 2, 16, 16, 48), 4))
    with pytest.raises(RuntimeError, match="multiple of 64"):
        ops.stem_plan_query_bf16(stem_desc((1, 1, 8, 8, 64), 8))
    with pytest.raises(RuntimeError, match="width"):
        ops.stem_plan_query_bf16(stem_desc((1, 4, 16, 6, 64), 8))
    bm = C.c_int32(-7)
    assert L.mvg_stem_plan_query_split(stem_desc((1, 2, 16, 16, 48), 4), C.byref(bm), None, None, None, None, None) == -1 and bm.value == -7


def test_stem_tables_agree_with_the_restated_launch_rules():
    """The forward forms of the table against the rule restated in prep_forms_ref at the two CU counts the GPU test sets (every
    CU of a 256-CU device, 8 CUs); the library's own answer for the CU-independent parts, and for the whole plan where this
    host's planner sees a device."""
    from rot_mvgaze_amd import ops
    for case, fwd, wg in R.SPLIT_STEM_CASES:
        for cus, want in zip((256, 8), fwd):
            assert R.split_stem_plan(case, cus) == (want, wg), (case, cus)
        got = ops.stem_plan_query_split(stem_desc(case, 4))
        assert got["wgrad"] == wg and got["fwd"][:2] == fwd[0][:2], (case, got)
    for case, fwd, wg in R.BF16_STEM_CASES:
        G, N, H, W, cout = case
        ho, wo = R.stem_out(H, W)
        assert (N * ho * (wo // 2)) % 64 == 0 and W % 4 == 0
        assert R.bf16_stem_plan(case) == (fwd, wg)
        got = ops.stem_plan_query_bf16(stem_desc(case, 8))
        rows = N * ho * (wo // 2)
        assert (got["fwd"]["kernel"], got["fwd"]["bn"]) == fwd and got["wgrad"] == wg, (case, got)
        assert (got["fwd"]["bm"], got["fwd"]["bk"], got["fwd"]["cls_kt"]) == (128, 64, [7])
        assert got["fwd"]["cls_tiles"] == [G * -(-rows // 128) * -(-2 * cout // got["fwd"]["bn"])]
    assert R.table_forms() == R.FORMS
    big = R.SPLIT_STEM_BIG
    ho, wo = R.stem_out(big[2], big[3])
    assert big[1] * ho * wo == 67032 and 67032 % 256 == 216
