"""CPU-side checks of the eval-mode BatchNorm backward's C ABI: both entry points (and the workspace query) are
declared in include/rotmvgaze.h (exported and bound type for type: tests/test_cabi_cpu.py, for every function) and wrapped in ops."""
import cabi_header as hdr
import rot_mvgaze_amd  # noqa: F401

NAMES = ("mvg_bn_eval_bwd", "mvg_bn_relu_maxpool_eval_bwd", "mvg_bn_eval_bwd_workspace_floats")


def test_eval_backward_entry_points_declared_exported_and_bound():
    for name in NAMES:
        assert name in hdr.functions, f"{name} is not declared in include/rotmvgaze.h"


def test_eval_backward_ops_wrappers_exist():
    from rot_mvgaze_amd import ops
    assert callable(ops.bn_eval_bwd) and callable(ops.bn_relu_maxpool_eval_bwd)
