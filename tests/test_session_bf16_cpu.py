"""The bf16 form of the inference session, host side (no GPU): the ABI additions, the fp32 plan left as it was, the bf16
plan's step order against a list derived here from arch.py's spec and heads.py's layer shapes, the tensor list, the rejected
configurations, and the bf16 plan's buffers checked by a stand-alone program under AddressSanitizer + UBSan (a plain
executable: nothing is loaded into Python and nothing is preloaded)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import cabi_header as hdr
import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd import arch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("mvg_session_create_ex", "mvg_session_compute", "mvg_session_num_steps", "mvg_session_step_name")
FP32, BF16 = 0, 1
CFG_FIELDS = ["depth", "num_iter", "views", "batch", "height", "width", "share_weights", "ignore_rotmat", "split", "raw_u8", "in_h",
              "in_w", "input_bgr"]


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from rot_mvgaze_amd import _lib
    return _lib.lib()


def _cfg(**kw):
    from rot_mvgaze_amd._lib import SessionCfg
    d = dict(depth=50, num_iter=3, views=2, batch=2, height=64, width=64, share_weights=0, ignore_rotmat=0, split=1, raw_u8=0,
             in_h=0, in_w=0, input_bgr=0)
    d.update(kw)
    return SessionCfg(**d)


class _Session:
    """compute None: mvg_session_create; FP32 / BF16: mvg_session_create_ex."""

    def __init__(self, L, compute, **kw):
        self.L, self.h = L, C.c_void_p()
        if compute is None:
            self.rc = L.mvg_session_create(C.byref(_cfg(**kw)), C.byref(self.h))
        else:
            self.rc = L.mvg_session_create_ex(C.byref(_cfg(**kw)), compute, C.byref(self.h))

    def __enter__(self):
        assert self.rc == 0, self.L.mvg_last_error()
        return self

    def __exit__(self, *exc):
        self.L.mvg_session_destroy(self.h)

    def names(self):
        return [self.L.mvg_session_tensor_name(self.h, i).decode() for i in range(self.L.mvg_session_num_tensors(self.h))]

    def numels(self):
        return [self.L.mvg_session_tensor_numel(self.h, i) for i in range(self.L.mvg_session_num_tensors(self.h))]

    def steps(self):
        n = self.L.mvg_session_num_steps(self.h)
        assert self.L.mvg_session_step_name(self.h, n) is None and self.L.mvg_session_step_name(self.h, -1) is None
        return [self.L.mvg_session_step_name(self.h, i).decode() for i in range(n)]

    def workspace(self):
        return self.L.mvg_session_workspace_bytes(self.h)

    def launches(self):
        return self.L.mvg_session_launches(self.h)


# ---------------------------------------------------------------- 1. symbols
def test_symbols(L):
    from rot_mvgaze_amd import _lib
    assert (hdr.constants["MVG_SESSION_FP32"], hdr.constants["MVG_SESSION_BF16"]) == (_lib.SESSION_FP32, _lib.SESSION_BF16) == (FP32, BF16)
    for name in NEW_ENTRY_POINTS:
        assert name in hdr.functions, f"{name} is not declared in include/rotmvgaze.h"
    # mvg_session_cfg is field for field what it was: the compute form is an argument of create_ex, not a field
    assert hdr.structs["mvg_session_cfg"] == [(n, "int32_t", None) for n in CFG_FIELDS]
    assert "the bf16 storage path, training" not in hdr.text     # the "Not representable" sentence no longer lists it
    assert L.mvg_session_compute(None) == -1 and L.mvg_session_num_steps(None) == -1


# ---------------------------------------------------------------- 2. the fp32 plan is what mvg_session_create builds
# Per fp32 op, the entry point its step calls ("memset": the split head path's slot clear, a stream-ordered memset)
FP32_STEP_NAMES = {"nchw_to_nhwc4", "preprocess_u8hwc_resize", "conv_fprop_affine", "conv_fprop_split_affine", "maxpool3x3s2_fwd",
                   "split_f32", "avgpool_fwd", "avgpool_fwd_split_scaled", "linear_fprop", "fuser_fprop", "linear_skinny_fwd",
                   "relative_rotation", "memset", "absmax_multi", "fuse_build_split", "linear_fprop_split"}


@pytest.mark.parametrize("depth", [18, 50])
def test_fp32_plan_unchanged(L, depth):
    n = 0
    for kw in (dict(), dict(split=0), dict(views=4, batch=86), dict(raw_u8=1, in_h=80, in_w=72), dict(share_weights=1),
               dict(height=224, width=224, batch=700)):
        with _Session(L, None, depth=depth, **kw) as a, _Session(L, FP32, depth=depth, **kw) as b:
            assert L.mvg_session_compute(a.h) == L.mvg_session_compute(b.h) == FP32
            assert a.names() == b.names() and a.numels() == b.numels()
            assert a.workspace() == b.workspace() and a.launches() == b.launches()
            assert a.steps() == b.steps() and len(a.steps()) == a.launches()
            assert set(a.steps()) <= FP32_STEP_NAMES
            assert L.mvg_session_num_range_units(a.h) == L.mvg_session_num_range_units(b.h)
            n += 1
    assert n == 6
    # the first steps of the default plan, by name: V input launches, the stem, the pool, the split of the pooled map
    with _Session(L, FP32, depth=depth) as s:
        assert s.steps()[:5] == ["nchw_to_nhwc4"] * 2 + ["conv_fprop_affine", "maxpool3x3s2_fwd", "split_f32"]
        assert s.steps()[-1] == "linear_skinny_fwd"


# ---------------------------------------------------------------- 3. the bf16 plan's order
def _mixed_mlp(fins_fouts):
    """heads._Mlp.forward on a Family.BF16 call over layers (fin, fout): Launch.BF16 unless the layer is padded (a width that is
    no multiple of 4 -> linear_fprop on zero-padded copies) or it is the last layer with fout <= 4 (linear_skinny_fwd)."""
    out = []
    for l, (fin, fout) in enumerate(fins_fouts):
        last = l == len(fins_fouts) - 1
        padded = fin % 4 != 0 or (fout % 4 != 0 and not (last and fout <= 4))
        if not padded and not (last and fout <= 4):
            out.append("linear_fprop_mixed")
        elif last and fout <= 4:
            out.append("linear_skinny_fwd")
        else:
            out.append("linear_fprop")
    return out


def _expected_bf16_steps(depth, views, raw, num_iter=3):
    spec = arch.backbone_spec(depth)
    cf, rot_dim = spec.fc_dim, arch.ROT_DIM
    steps = ["preprocess_u8hwc_resize_bf16" if raw else "nchw_to_nhwc8_bf16"] * views        # Backbone._input_layout
    steps += ["conv_fprop_bf16", "bn_relu_maxpool_fwd_bf16"]                                # the stem through _unit_fwd(pool=True)
    for blk in spec.blocks:                                                                 # Backbone._forward_infer
        steps += ["conv_fprop_bf16_affine"] * (len(blk.convs) - 1)                          # conv1 .. the last but one
        if blk.downsample is not None:
            steps.append("conv_fprop_bf16_affine")                                          # the downsample branch, no ReLU
        steps.append("conv_fprop_bf16_affine")                                              # the last conv, residual + ReLU
    steps.append("avgpool_fwd_bf16")
    kin = cf + rot_dim                                                                      # FusionHead.forward, mixed
    steps += _mixed_mlp([(cf, rot_dim), (rot_dim, rot_dim)])                                # the lifter
    steps.append("relative_rotation")
    for _ in range(num_iter):
        steps += ["rotcat_fwd"] + _mixed_mlp([(kin, kin), (kin, rot_dim)])                  # _fuser_input, the fuser
        steps += ["rotcat_fwd"] + _mixed_mlp([(kin, 512), (512, 2)])                        # _head_input, the head
    return steps


@pytest.mark.parametrize("depth", [18, 50])
@pytest.mark.parametrize("views", [2, 3])
def test_bf16_plan_order(L, depth, views):
    nconv = {18: 20, 50: 53}[depth]
    for raw in (0, 1):
        for share in (0, 1):
            kw = dict(depth=depth, views=views, batch=2, height=64, width=64, raw_u8=raw, in_h=80 * raw, in_w=72 * raw,
                      share_weights=share)
            with _Session(L, BF16, **kw) as s:
                assert L.mvg_session_compute(s.h) == BF16
                steps = s.steps()
                assert steps == _expected_bf16_steps(depth, views, raw)
                assert steps.count("conv_fprop_bf16_affine") == nconv - 1
                for name in steps:
                    assert "split" not in name and ("_affine" not in name or "bf16" in name), name
                assert L.mvg_session_num_range_units(s.h) == 0 and L.mvg_session_range_unit_name(s.h, 0) is None
                # the rule, both forms: mvg_session_launches counts the plan's steps - one library call (or the one memset of
                # the fp32 split head path) each; nothing is added on top
                assert s.launches() == len(steps)
                # split is accepted and ignored
                with _Session(L, BF16, **dict(kw, split=0)) as t:
                    assert t.steps() == steps and t.workspace() == s.workspace()
                # no range record can be set, as on a split = 0 session; clearing one is fine
                word = C.c_uint32(0)
                assert L.mvg_session_set_range_record(s.h, C.byref(word)) != 0 and L.mvg_last_error()
                assert L.mvg_session_set_range_record(s.h, None) == 0


# ---------------------------------------------------------------- 4. tensors
@pytest.mark.parametrize("depth", [18, 50])
def test_bf16_tensor_names_match_the_state_dict(L, depth):
    from rot_mvgaze_amd.model import FeatRotationSymm
    sd = FeatRotationSymm(depth, 3).state_dict()
    want = [k for k in sd if not k.startswith("_feat_extractor.0.fc.") and not k.endswith("num_batches_tracked")]
    shared = [k for k in want if not re.match(r"_(img_fusers|gaze_estimators)\.[12]\.", k)]
    assert len(shared) == len(want) - 16
    for views in (2, 3):
        for raw in (0, 1):
            with _Session(L, BF16, depth=depth, views=views, raw_u8=raw, in_h=80 * raw, in_w=72 * raw) as s, \
                    _Session(L, FP32, depth=depth, views=views) as f:
                assert s.names() == want == f.names()
                assert s.numels() == [sd[k].numel() for k in want]
    with _Session(L, BF16, depth=depth, share_weights=1) as s:
        assert s.names() == shared
        assert s.numels() == [sd[k].numel() for k in shared]


# ---------------------------------------------------------------- 5. rejections
@pytest.mark.parametrize("compute,bad", [(2, dict()), (-1, dict()), (BF16, dict(depth=34)), (BF16, dict(views=1)), (BF16, dict(batch=0)),
                                         (BF16, dict(raw_u8=1, in_h=0, in_w=72)), (FP32, dict(depth=34)),
                                         # a shape the stem's bf16 pooling pass rejects (views x batch x pooled rows >= 65536)
                                         (BF16, dict(views=8, batch=147, height=224, width=224))])
def test_rejected_configurations(L, compute, bad):
    h = C.c_void_p(1)
    rc = L.mvg_session_create_ex(C.byref(_cfg(**bad)), compute, C.byref(h))
    assert rc != 0 and h.value is None
    assert L.mvg_last_error()


def test_rejected_null_arguments(L):
    h = C.c_void_p(1)
    assert L.mvg_session_create_ex(None, BF16, C.byref(h)) != 0 and h.value is None and L.mvg_last_error()
    assert L.mvg_session_create_ex(C.byref(_cfg()), BF16, None) != 0 and L.mvg_last_error()


# ---------------------------------------------------------------- 6. the plan, stand-alone under the sanitizers
def test_bf16_plan_standalone_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed to build tests/native/session_bf16_plan_check.cpp"
    exe = str(tmp_path / "session_bf16_plan_check")
    # the sanitizer runtimes are linked into the executable: it runs as it is, with nothing preloaded
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static + ["-o", exe,
                    os.path.join(ROOT, "tests", "native", "session_bf16_plan_check.cpp"),
                    os.path.join(ROOT, "rot-mvgaze_amd", "csrc", "session_plan.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "session_bf16_plan_check: ok" in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
