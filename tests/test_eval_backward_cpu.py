"""CPU-side checks of the eval-mode BatchNorm backward's C ABI: both entry points (and the workspace query) are
declared in include/rotmvgaze.h, exported by the library and bound in _lib.SIGNATURES with the header's arity."""
import os
import re

import pytest

import rot_mvgaze_amd  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mvg_bn_eval_bwd", "mvg_bn_relu_maxpool_eval_bwd", "mvg_bn_eval_bwd_workspace_floats")


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from rot_mvgaze_amd import _lib
    return _lib.lib()


def _declarations():
    hdr = open(os.path.join(ROOT, "include", "rotmvgaze.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(mvg_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)}


def test_eval_backward_entry_points_declared_exported_and_bound(built_lib):
    from rot_mvgaze_amd import _lib
    decl = _declarations()
    for name in NAMES:
        assert name in decl, f"{name} is not declared in include/rotmvgaze.h"
        assert hasattr(built_lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
        nargs = len([a for a in decl[name].split(",") if a.strip()])
        assert len(_lib.SIGNATURES[name][1]) == nargs, (name, nargs, len(_lib.SIGNATURES[name][1]))
    assert _lib.ABI_VERSION == 13


def test_eval_backward_ops_wrappers_exist():
    from rot_mvgaze_amd import ops
    assert callable(ops.bn_eval_bwd) and callable(ops.bn_relu_maxpool_eval_bwd)
