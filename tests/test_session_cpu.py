"""The inference session's host side (no GPU): the ABI additions, the tensor list against the module's state_dict, the
buffer plan's reuse, where the head path switches, the rejected configurations, and the plan builder compiled stand-alone
under AddressSanitizer + UBSan (a plain executable: nothing is loaded into Python and nothing is preloaded)."""
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
SESSION_ENTRY_POINTS = ("mvg_session_create", "mvg_session_destroy", "mvg_session_num_tensors", "mvg_session_tensor_name",
                        "mvg_session_tensor_numel", "mvg_session_workspace_bytes", "mvg_session_launches", "mvg_session_bind",
                        "mvg_session_forward", "mvg_bn_eval_affine_batch")


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
    def __init__(self, L, **kw):
        self.L, self.h = L, C.c_void_p()
        self.rc = L.mvg_session_create(C.byref(_cfg(**kw)), C.byref(self.h))

    def __enter__(self):
        assert self.rc == 0, self.L.mvg_last_error()
        return self

    def __exit__(self, *exc):
        self.L.mvg_session_destroy(self.h)

    def names(self):
        return [self.L.mvg_session_tensor_name(self.h, i).decode() for i in range(self.L.mvg_session_num_tensors(self.h))]

    def numels(self):
        return [self.L.mvg_session_tensor_numel(self.h, i) for i in range(self.L.mvg_session_num_tensors(self.h))]

    def workspace(self):
        return self.L.mvg_session_workspace_bytes(self.h)

    def launches(self):
        return self.L.mvg_session_launches(self.h)


def test_abi_additions():
    """The session's entry points are in the header (how each is exported and bound: tests/test_cabi_cpu.py, for every function)."""
    for name in SESSION_ENTRY_POINTS:
        assert name in hdr.functions, f"{name} is not declared in include/rotmvgaze.h"


@pytest.mark.parametrize("depth", [18, 50])
def test_tensor_names_match_the_state_dict(L, depth):
    from rot_mvgaze_amd.model import FeatRotationSymm
    sd = FeatRotationSymm(depth, 3).state_dict()
    want = [k for k in sd if not k.startswith("_feat_extractor.0.fc.") and not k.endswith("num_batches_tracked")]
    shared = [k for k in FeatRotationSymm(depth, 3, share_weights=True).state_dict()
              if not k.startswith("_feat_extractor.0.fc.") and not k.endswith("num_batches_tracked")
              and not re.match(r"_(img_fusers|gaze_estimators)\.[12]\.", k)]
    assert len(shared) == len(want) - 16
    n = 0
    for views in (2, 3, 4):
        for batch in (1, 3, 86):
            for hw in (64, 224):
                for split in (0, 1):
                    for raw in (0, 1):
                        with _Session(L, depth=depth, views=views, batch=batch, height=hw, width=hw, split=split, raw_u8=raw,
                                      in_h=80 * raw, in_w=72 * raw) as s:
                            assert s.names() == want
                            assert s.numels() == [sd[k].numel() for k in want]
                            n += 1
    assert n == 72
    with _Session(L, depth=depth, share_weights=1) as s:
        assert s.names() == shared
        assert s.numels() == [sd[k].numel() for k in shared]


def _unit_output_elems_per_image(depth, hw):
    """Every conv + BatchNorm unit's output elements for one image (the no-reuse yardstick)."""
    spec = arch.backbone_spec(depth)
    size = lambda h, c: (h + 2 * c.pad - c.k) // c.stride + 1
    h = size(hw, spec.stem)
    total = h * h * spec.stem.cout
    h = (h + 2 - 3) // 2 + 1
    for blk in spec.blocks:
        hb = h
        for c in blk.convs:
            hb = size(hb, c)
            total += hb * hb * c.cout
        if blk.downsample is not None:
            hd = size(h, blk.downsample)
            total += hd * hd * blk.downsample.cout
        h = hb
    return total


def test_workspace_reuses_buffers(L):
    sizes = []
    for batch in (1, 2, 8, 32, 85, 86, 128):
        with _Session(L, depth=50, views=4, batch=batch, height=224, width=224) as s:
            sizes.append(s.workspace())
    assert sizes == sorted(sizes) and sizes[0] > 0
    per_image = _unit_output_elems_per_image(50, 224)
    assert abs(per_image - 11.114e6) < 0.001e6
    no_reuse = per_image * 4 * 128 * 4                       # C3 eval: R50, V = 4, B = 128, fp32 / sp = 4 bytes per element
    assert sizes[-1] <= no_reuse / 2, (sizes[-1], no_reuse)


def test_head_path_switches_at_1024_rows(L):
    with _Session(L, depth=18, views=4, batch=85) as a, _Session(L, depth=18, views=4, batch=86) as b:
        assert a.launches() > 0 and b.launches() > 0
        assert a.launches() != b.launches()                  # 1020 rows: generated-input fp32-MFMA Linears; 1032: the split Linears
    with _Session(L, depth=18, views=4, batch=85, split=0) as a, _Session(L, depth=18, views=4, batch=86, split=0) as b:
        assert a.launches() == b.launches()                  # MVG_SPLIT=0: one head path at every row count


@pytest.mark.parametrize("bad", [dict(depth=34), dict(views=1), dict(batch=0), dict(raw_u8=1, in_h=0, in_w=72), None])
def test_rejected_configurations(L, bad):
    h = C.c_void_p(1)
    rc = L.mvg_session_create(C.byref(_cfg(**bad)) if bad is not None else None, C.byref(h))
    assert rc != 0 and h.value is None
    assert L.mvg_last_error()


def test_split_head_serves_at_most_five_iterations(L):
    """The split head path's slot arena (11 slots per iteration plus 2 of 64) serves num_iter <= 5: from 1024 rows with split = 1
    a session of 6 is refused in words, 5 builds, and 6 builds wherever the head does not run on the split Linears (fewer rows,
    split = 0).  (The training head steps aside to its fp32 Linears instead: tests/test_iter_count_gpu.py.)"""
    from rot_mvgaze_amd.heads import FusionHead, SPLIT_MIN_ROWS
    assert [FusionHead.split_serves(i) for i in (1, 5, 6, 7)] == [True, True, False, False]
    big = dict(depth=18, views=4, batch=96)                   # 4 * 3 * 96 = 1152 rows
    assert 12 * 96 >= SPLIT_MIN_ROWS > 12 * 85
    h = C.c_void_p(1)
    assert L.mvg_session_create(C.byref(_cfg(num_iter=6, split=1, **big)), C.byref(h)) != 0 and h.value is None
    msg = L.mvg_last_error().decode()
    assert msg == "session_create: num_iter 6 is more than the split head path's slot arena serves (at most 5)", msg
    with _Session(L, num_iter=5, split=1, **big) as s:
        assert s.launches() > 0
    with _Session(L, num_iter=6, split=0, **big) as a, _Session(L, num_iter=6, split=1, depth=18, views=4, batch=85) as b:
        assert a.launches() > 0 and b.launches() > 0


def _build_standalone(tmp_path, name):
    """tests/native/<name>.cpp and session_plan.cpp, and nothing else, as one executable under ASan + UBSan."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, f"a host C++ compiler is needed to build tests/native/{name}.cpp"
    exe = str(tmp_path / name)
    # the sanitizer runtimes are linked into the executable: it runs as it is, with nothing preloaded
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static + ["-o", exe,
                    os.path.join(ROOT, "tests", "native", name + ".cpp"),
                    os.path.join(ROOT, "rot-mvgaze_amd", "csrc", "session_plan.cpp")], check=True)
    return exe


def test_plan_builder_standalone_under_sanitizers(tmp_path):
    r = subprocess.run([_build_standalone(tmp_path, "session_plan_check")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "session_plan_check: ok" in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr


def test_plans_match_the_recorded_digests(tmp_path):
    """Every field of every plan over the dump's sweep (both depths, 2 / 3 / 8 views, batch up to 700, 64 and 224 px, the
    fp32-MFMA, split and bf16 forms, raw_u8 / share_weights / ignore_rotmat, num_iter 1 .. 6, 32 px, 96 x 64) is what
    tests/golden/session_plan_digests.txt records, and the rejected configurations are rejected with the recorded text: the
    executor reads nothing but the plan, so the forward a session queues has not moved.

    A change that means to move the plan regenerates the fixture from its own build and says so:
        g++ -std=c++17 -O1 -o /tmp/session_plan_dump tests/native/session_plan_dump.cpp rot-mvgaze_amd/csrc/session_plan.cpp
        /tmp/session_plan_dump > tests/golden/session_plan_digests.txt
    (`session_plan_dump --full` prints the rendering behind each digest; diff two of them to see what moved.)"""
    r = subprocess.run([_build_standalone(tmp_path, "session_plan_dump")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    want = open(os.path.join(ROOT, "tests", "golden", "session_plan_digests.txt")).read()
    got, exp = r.stdout.splitlines(), want.splitlines()
    moved = [f"{g!r} (recorded: {e!r})" for g, e in zip(got, exp) if g != e]
    assert r.stdout == want, f"{len(got)} lines against {len(exp)} recorded; {len(moved)} differ, the first: {moved[:3]}"
