"""Host side of the inference range guard (no GPU): the new entry points are declared in include/rotmvgaze.h next to the
unchanged ones they extend (tests/test_cabi_cpu.py holds every function's export and binding, and the one pin of
MVG_ABI_VERSION); arch.range_unit_names is the session's list;
a session off the split kernels has no range units; setting a record moves nothing in the plan; and the plan's word indices,
checked by a stand-alone program built with the plan builder alone under AddressSanitizer + UBSan (a plain executable:
nothing is loaded into Python and nothing is preloaded)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import cabi_header as hdr
import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd import arch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mvg_conv_fprop_split_affine_ranged", "mvg_split_f32_ranged", "mvg_session_num_range_units", "mvg_session_range_unit_name",
       "mvg_session_set_range_record")
# the entry points these extend keep their signatures
UNCHANGED = {"mvg_conv_fprop_split_affine": 13, "mvg_split_f32": 5, "mvg_session_forward": 8, "mvg_session_create": 2}


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from rot_mvgaze_amd import _lib
    return _lib.lib()


def _cfg(**kw):
    from rot_mvgaze_amd._lib import SessionCfg
    d = dict(depth=18, num_iter=3, views=2, batch=2, height=64, width=64, share_weights=0, ignore_rotmat=0, split=1, raw_u8=0,
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

    def range_names(self):
        n = self.L.mvg_session_num_range_units(self.h)
        assert self.L.mvg_session_range_unit_name(self.h, n) is None and self.L.mvg_session_range_unit_name(self.h, -1) is None
        return [self.L.mvg_session_range_unit_name(self.h, i).decode() for i in range(n)]


def test_range_entry_points_declared_exported_and_bound():
    for name in NEW + tuple(UNCHANGED):
        assert name in hdr.functions, f"{name} is not declared in include/rotmvgaze.h"
    for name, arity in UNCHANGED.items():
        assert hdr.arity(name) == arity, f"{name} changed its signature"
    # the ranged entry points are the old ones plus the word, in front of the stream
    assert hdr.arity("mvg_conv_fprop_split_affine_ranged") == UNCHANGED["mvg_conv_fprop_split_affine"] + 1
    assert hdr.arity("mvg_split_f32_ranged") == UNCHANGED["mvg_split_f32"] + 1
    from rot_mvgaze_amd import ops
    assert callable(ops.conv_fprop_split_affine_ranged) and callable(ops.split_f32_ranged)


def test_required_arguments_are_checked_on_the_host(L):
    """A null word / an fp32 output is refused before anything is launched (no GPU is touched)."""
    from rot_mvgaze_amd._lib import ConvDesc
    d = ConvDesc.make(1, 2, 8, 8, 32, 64, 1, 1, 0)
    one = C.c_void_p(16)
    assert L.mvg_conv_fprop_split_affine_ranged(C.byref(d), one, None, one, one, one, 1, one, one, None, 0, 1, None, None) != 0
    assert b"range_word" in L.mvg_last_error()
    assert L.mvg_conv_fprop_split_affine_ranged(C.byref(d), one, None, one, one, one, 0, one, one, None, 0, 1, one, None) != 0
    assert b"out_sp" in L.mvg_last_error()
    assert L.mvg_split_f32_ranged(one, one, 8, 1.0, None, None) != 0
    assert L.mvg_split_f32_ranged(one, one, 12, 1.0, one, None) != 0


@pytest.mark.parametrize("depth,count", [(18, 17), (50, 49)])
def test_range_unit_names(L, depth, count):
    names = arch.range_unit_names(depth)
    spec = arch.backbone_spec(depth)
    assert len(names) == count == 1 + sum(len(b.convs) for b in spec.blocks) and len(set(names)) == count
    assert names[0] == spec.stem.name and names[1] == spec.blocks[0].convs[0].name and names[-1] == spec.blocks[-1].convs[-1].name
    assert not any("downsample" in n for n in names)
    for views, batch, hw in ((2, 2, 64), (3, 1, 96), (4, 86, 64), (2, 8, 224)):
        with _Session(L, depth=depth, views=views, batch=batch, height=hw, width=hw) as s:
            assert s.range_names() == names


def test_no_range_units_off_the_split_kernels(L):
    with _Session(L, depth=18, split=0) as s:
        assert s.range_names() == []
    with _Session(L, depth=50, split=0, height=224, width=224) as s:
        assert s.range_names() == []
    # The 2 GiB guard (Backbone.forward, session_plan.cpp): one view of layer1's output, 4 bytes per element, must stay below
    # 0x7FFFFFF0 bytes.  ResNet-50 at 224 px: 56 x 56 x 256 x 4 = 3 211 264 bytes per image - batch 668 is the LAST one that fits
    # (2 145 124 352 bytes), batch 669 is past the guard
    fits = lambda batch: 4 * batch * 56 * 56 * 256 < 0x7FFFFFF0
    assert fits(668) and not fits(669)
    for batch in (667, 668, 669, 700):
        with _Session(L, depth=50, batch=batch, height=224, width=224) as s:
            assert len(s.range_names()) == (49 if fits(batch) else 0), batch
            if not fits(batch):
                assert L.mvg_session_set_range_record(s.h, C.c_void_p(256)) != 0 and L.mvg_last_error()


def test_set_range_record_only_stores_the_pointer(L):
    for kw in (dict(depth=18), dict(depth=50, views=4, batch=86)):
        with _Session(L, **kw) as s:
            before = (L.mvg_session_launches(s.h), L.mvg_session_workspace_bytes(s.h), L.mvg_session_num_tensors(s.h))
            assert L.mvg_session_set_range_record(s.h, C.c_void_p(4096)) == 0           # a host-only handle: never dereferenced
            assert (L.mvg_session_launches(s.h), L.mvg_session_workspace_bytes(s.h), L.mvg_session_num_tensors(s.h)) == before
            assert L.mvg_session_set_range_record(s.h, None) == 0
            assert L.mvg_session_launches(s.h) == before[0]


def test_range_indices_standalone_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed to build tests/native/session_range_check.cpp"
    exe = str(tmp_path / "session_range_check")
    # the sanitizer runtimes are linked into the executable: it runs as it is, with nothing preloaded
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static + ["-o", exe,
                    os.path.join(ROOT, "tests", "native", "session_range_check.cpp"),
                    os.path.join(ROOT, "rot-mvgaze_amd", "csrc", "session_plan.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "session_range_check: ok" in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr


def test_guard_attribute_defaults_and_state_dict():
    """The guard is off by default and adds nothing to the state_dict (the record is a plain attribute)."""
    from rot_mvgaze_amd.backbone import Backbone
    from rot_mvgaze_amd.model import FeatRotationSymm
    m = FeatRotationSymm(18, 3)
    assert m.split_eval_guard is None
    assert not any("range" in k for k in m.state_dict())
    bb = Backbone(18, dict(m.named_parameters()))
    assert bb.split_eval_guard is None and bb._range_record is None
    assert list(bb._range_slot) == arch.range_unit_names(18)
    with pytest.raises(RuntimeError):
        bb.range_report()
