"""CPU-side checks of the boundary: the C-ABI library builds, loads and exports every symbol the
header declares; the ctypes binding (_lib.SIGNATURES, the Structure mirrors, the constants, augment.REC_DTYPE) agrees with
the header type for type and every call site passes the declared number of arguments; the drop-in module honours the reference's checkpoint contract; the pair index
(host integer code inside the library) is bit-exact with the reference's fixtures; the product
fails loudly without a GPU instead of falling back."""
import ast
import ctypes as C
import glob
import json
import os

import numpy as np
import pytest
import torch

import cabi_header as hdr
import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd import arch, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from rot_mvgaze_amd import _lib
    return _lib.lib()


# ---------------------------------------------------------------- the binding against the header (tests/cabi_header.py)
SCALAR_CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "size_t": C.c_size_t, "float": C.c_float,
                 "double": C.c_double, "uint8_t": C.c_uint8, "uint16_t": C.c_uint16, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
# every struct the header defines -> its Python mirror (a ctypes.Structure of _lib, or augment's numpy record)
STRUCT_MIRRORS = {"mvg_conv_desc": "ConvDesc", "mvg_conv_plan": "ConvPlan", "mvg_bn_plan": "BnPlan", "mvg_prof_entry": "ProfEntry",
                  "mvg_session_cfg": "SessionCfg", "mvg_augment_rec": "augment.REC_DTYPE"}


def _mirror(struct):
    from rot_mvgaze_amd import _lib, augment
    owner, _, attr = STRUCT_MIRRORS[struct].rpartition(".")
    return getattr(augment if owner == "augment" else _lib, attr)


def _binds(ctype, bound):
    """Whether ctypes type `bound` (None: no value) may stand for the header's C type (cabi_header's spelling)."""
    base, stars = ctype.rstrip("*"), ctype.count("*")
    if stars == 0:
        return bound is (None if base == "void" else SCALAR_CTYPES[base])
    if ctype == "char*":
        return bound is C.c_char_p
    if bound is C.c_void_p:
        return True
    if not (isinstance(bound, type) and issubclass(bound, C._Pointer)):
        return False                                             # a pointer is never bound as a scalar
    if stars == 2:
        return bound._type_ is C.c_void_p
    if base in SCALAR_CTYPES:
        return bound._type_ is SCALAR_CTYPES[base]
    mirror = _mirror(base) if hdr.structs.get(base) else None     # an opaque struct travels as c_void_p only
    return isinstance(mirror, type) and bound._type_ is mirror


def test_header_symbols_exported(built_lib):
    from rot_mvgaze_amd import _lib
    assert len(hdr.functions) >= 35
    for name in hdr.functions:
        assert hasattr(built_lib, name), f"{name} declared in include/rotmvgaze.h but not exported"
    # the one literal pin of the version: header, binding and built library
    assert hdr.constants["MVG_ABI_VERSION"] == _lib.ABI_VERSION == built_lib.mvg_abi_version() == 13


def test_every_signature_matches_the_header_type_for_type():
    from rot_mvgaze_amd import _lib
    assert set(hdr.functions) == set(_lib.SIGNATURES), set(hdr.functions) ^ set(_lib.SIGNATURES)
    for name, (ret, params) in hdr.functions.items():
        res, args = _lib.SIGNATURES[name]
        assert _binds(ret, res), f"{name}: returns {ret} in the header, bound as {res}"
        assert len(args) == len(params), f"{name}: {len(params)} parameters in the header, {len(args)} bound"
        for k, ((ctype, pname), bound) in enumerate(zip(params, args)):
            assert _binds(ctype, bound), f"{name}: argument {k} ({ctype} {pname}) is bound as {getattr(bound, '__name__', bound)}"


def _same_fields(struct, got, want):
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{struct}: field {k} is {w} in the header, {g} in {STRUCT_MIRRORS[struct]}"
    assert len(got) == len(want), f"{struct}: {len(want)} fields in the header, {len(got)} in {STRUCT_MIRRORS[struct]}"


def test_every_struct_matches_its_mirror():
    defined = {name for name, fields in hdr.structs.items() if fields is not None}
    assert defined == set(STRUCT_MIRRORS), f"structs without a mirror named here (or mirrors of nothing): {defined ^ set(STRUCT_MIRRORS)}"
    assert [name for name, fields in hdr.structs.items() if fields is None] == ["mvg_session"]
    for struct in sorted(defined):
        want = [(n, SCALAR_CTYPES[base], length) for n, base, length in hdr.structs[struct]]
        mirror = _mirror(struct)
        if isinstance(mirror, np.dtype):
            got = [(n, mirror.fields[n][0].base, mirror.fields[n][0].shape) for n in mirror.names]
            _same_fields(struct, got, [(n, np.dtype(t), (length,) if length else ()) for n, t, length in want])
            offset = align = 0                                   # natural C alignment of the header's fields
            for n, t, length in want:
                offset = -(-offset // C.alignment(t)) * C.alignment(t)
                assert mirror.fields[n][1] == offset, f"{struct}.{n}: at {mirror.fields[n][1]}, C puts it at {offset}"
                offset += C.sizeof(t) * (length or 1)
                align = max(align, C.alignment(t))
            assert mirror.itemsize == -(-offset // align) * align, f"{struct}: itemsize {mirror.itemsize}"
        else:
            got = [(n, t._type_, t._length_) if issubclass(t, C.Array) else (n, t, None) for n, t in mirror._fields_]
            _same_fields(struct, got, want)


def test_every_constant_matches_the_header():
    from rot_mvgaze_amd import _lib
    mine = {name: v for name, v in vars(_lib).items() if name.isupper() and isinstance(v, int)}
    assert {"K_FAMILIES", "ABI_VERSION", "SESSION_BF16", "PLAN_DGRAD", "BN_PASS_FINALIZE", "BN_ELEM_SP", "BN_MERGE_PER_GROUP"} <= set(mine)
    for name, v in mine.items():
        assert hdr.constants.get("MVG_" + name) == v, f"_lib.{name} = {v}, the header's MVG_{name} = {hdr.constants.get('MVG_' + name)}"
    for prefix in ("MVG_SESSION_", "MVG_PLAN_", "MVG_BN_PASS_", "MVG_BN_ELEM_", "MVG_BN_MERGE_"):        # and none left unbound
        for name in hdr.constants:
            assert not name.startswith(prefix) or name[4:] in mine, f"{name} has no counterpart in _lib"


# ---------------------------------------------------------------- call sites
def _callees(node):
    """The entry points a call's callee expression may name: x.mvg_y, _fn("mvg_y", t) (mvg_y or mvg_y_bf16), or a
    conditional between two such.  None: not a call into the library."""
    if isinstance(node, ast.Attribute) and node.attr.startswith("mvg_"):
        return [node.attr]
    if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "_fn" and node.args \
            and isinstance(node.args[0], ast.Constant) and isinstance(node.args[0].value, str):
        return [node.args[0].value, node.args[0].value + "_bf16"]
    if isinstance(node, ast.IfExp):
        a, b = _callees(node.body), _callees(node.orelse)
        if a is None and b is None:
            return None
        assert a is not None and b is not None, f"line {node.lineno}: only one arm of the conditional is an entry point"
        return a + b
    return None


def test_every_call_site_passes_the_declared_arguments():
    from rot_mvgaze_amd import _lib
    files = sorted(glob.glob(os.path.join(ROOT, "rot-mvgaze_amd", "*.py")) + glob.glob(os.path.join(ROOT, "scripts", "*.py"))
                   + glob.glob(os.path.join(ROOT, "tests", "*.py")) + [os.path.join(ROOT, "bench.py")])
    calls = 0
    for path in files:
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for node in ast.walk(tree):
            names = _callees(node.func) if isinstance(node, ast.Call) else None
            for name in names or ():
                where = f"{os.path.relpath(path, ROOT)}:{node.lineno}: {name}"
                assert name in _lib.SIGNATURES, f"{where} is not in _lib.SIGNATURES"
                assert not node.keywords and not any(isinstance(a, ast.Starred) for a in node.args), f"{where}: keyword or * argument"
                want = len(_lib.SIGNATURES[name][1])
                assert len(node.args) == want, f"{where} takes {want} arguments, the call passes {len(node.args)}"
                calls += 1
    assert calls > 200                                           # ops.py and the tests hold some 140 each: the walk found them


def test_pair_index_bit_exact(built_lib, golden_dir):
    from rot_mvgaze_amd.pair_index import PairIndexRNG, build_pair_index
    with open(os.path.join(golden_dir, "pair_index.json")) as f:
        cases = json.load(f)
    n = 0
    for key, c in cases.items():
        if key == "shared_stream":
            rng = PairIndexRNG(c["seed"])
            assert [list(t) for t in build_pair_index(c["train_rows"], "novel_train", rng)] == c["train"]
            assert [list(t) for t in build_pair_index(c["test_rows"], "novel_test", rng)] == c["test"]
            continue
        got = build_pair_index(c["rows"], c["tag"], PairIndexRNG(c["seed"]))
        assert [list(t) for t in got] == c["tuples"], key
        n += len(got)
    assert n > 1000
    # edge cases: empty list, file shorter than a frame, single selected camera in a partial frame
    assert build_pair_index([], "all", PairIndexRNG(0)) == []
    assert build_pair_index([1], "all", PairIndexRNG(0)) == []
    assert build_pair_index([3], "novel_test", PairIndexRNG(0)) == []       # only camera 2 is selected
    # a larger run against the oracle restatement
    from oracle import restatement as R
    rows = [18 * 700 + 5, 18 * 123, 17]
    for tag in ("all", "novel_train", "novel_test"):
        assert build_pair_index(rows, tag, PairIndexRNG(42)) == R.build_pair_index(rows, tag, R.MT19937(42))


@pytest.mark.parametrize("depth", [18, 50])
def test_state_dict_contract(depth):
    from rot_mvgaze_amd.model import FeatRotationSymm
    m = FeatRotationSymm(backbone_depth=depth, num_iter=3)
    sd = m.state_dict()
    want = {n: tuple(s) for n, s, _ in arch.state_dict_shapes(depth, 3)}
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert len(sd) == (150 if depth == 18 else 348)
    nparam = sum(p.numel() for p in m.parameters())
    assert nparam == (40_019_502 if depth == 18 else 91_640_366)
    ref = synth.make_state_dict(depth, 3, 3, perturb_bn=True)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in ref.items()}, strict=True)
    back = m.state_dict()
    for k, v in ref.items():
        assert np.array_equal(back[k].numpy(), np.asarray(v)), k
    w = dict(m.named_parameters())["_feat_extractor.0.layer1.0.conv1.weight"]
    assert w.is_contiguous(memory_format=torch.channels_last)                # KRSC in memory


def test_invalid_variants_and_cpu_inputs_fail_loudly():
    from rot_mvgaze_amd.model import FeatRotationSymm
    with pytest.raises(AssertionError):                                   # rot_mv.py:133
        FeatRotationSymm(18, 3, encode_rotmat=True, ignore_rotmat=True)
    with pytest.raises(ValueError):                                       # combinations the reference cannot run either
        FeatRotationSymm(18, 3, share_feature=True, share_weights=True)
    m = FeatRotationSymm(18, 3)
    d = {"img_0": torch.zeros(1, 3, 32, 32), "img_1": torch.zeros(1, 3, 32, 32),
         "rot_0": torch.eye(3)[None], "rot_1": torch.eye(3)[None]}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(d)
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rotation_matrix_2d(torch.zeros(2, 2))


def test_missing_library_is_an_error(monkeypatch, tmp_path):
    from rot_mvgaze_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.lib()


def test_host_angular_error_metric(golden_dir):
    from rot_mvgaze_amd.geometry import angular_error
    g = np.load(os.path.join(golden_dir, "geometry_loss.npz"))
    sel = [0, 1] + list(range(3, 32))
    got = angular_error(g["loss_pred"].astype(np.float64), g["loss_gt"].astype(np.float64))
    np.testing.assert_allclose(got[sel], g["ang_err_np"][sel], rtol=1e-9, atol=1e-9)
