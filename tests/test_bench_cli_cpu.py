"""bench.py's options and its output dump, without a GPU: a plain run leaves the secondary figures to --full,
--steps is the number of timed steps, and --dump-outputs writes float32 arrays whose samples are fixed by
name and size and stay within the size budget.  The real run is in tests/test_bench_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_plain_run_defaults_and_full_flag():
    a = bench.build_parser().parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    a = bench.build_parser().parse_args(["--steps", "3", "--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_step_counts_are_checked(argv):
    with pytest.raises(SystemExit):
        bench.build_parser().parse_args(argv)


def test_dump_outputs_writes_float32_and_fixed_samples(tmp_path):
    g = torch.Generator().manual_seed(0)
    big = torch.randn(bench.DUMP_MAX_ELEMS + 12345, generator=g)
    arrays = {"pred_gaze": torch.randn(8, 2, generator=g), "feats": big, "loss": torch.tensor(0.5, dtype=torch.float64),
              "half": torch.randn(4, 3, generator=g).to(torch.bfloat16)}
    params = [("a.weight", torch.randn(64, 64, generator=g)), ("a.bias", torch.randn(5, generator=g))]
    names = bench.dump_outputs(str(tmp_path / "d1"), arrays, params=params, grads=params[:1])
    assert names == ["feats", "grad_sample", "half", "loss", "param_sample", "pred_gaze"]
    total = 0
    for n in names:
        a = np.load(tmp_path / "d1" / f"{n}.npy")
        assert a.dtype == np.float32
        total += a.nbytes
    assert total <= bench.DUMP_BUDGET_BYTES
    np.testing.assert_array_equal(np.load(tmp_path / "d1" / "pred_gaze.npy"), arrays["pred_gaze"].numpy())
    feats = np.load(tmp_path / "d1" / "feats.npy")
    idx = bench._dump_sample("feats", big.numel(), bench.DUMP_MAX_ELEMS)
    assert feats.shape == (bench.DUMP_MAX_ELEMS,) and len(np.unique(idx)) == idx.size
    np.testing.assert_array_equal(feats, big.numpy()[idx])
    ps = np.load(tmp_path / "d1" / "param_sample.npy")
    assert ps.shape == (min(64 * 64, bench.DUMP_PARAM_SAMPLE) + 5,)
    # same arrays -> the same files, byte for byte
    bench.dump_outputs(str(tmp_path / "d2"), arrays, params=params, grads=params[:1])
    for n in names:
        assert (tmp_path / "d1" / f"{n}.npy").read_bytes() == (tmp_path / "d2" / f"{n}.npy").read_bytes()


def test_dump_outputs_refuses_to_exceed_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1000)
    with pytest.raises(AssertionError, match="budget"):
        bench.dump_outputs(str(tmp_path), {"x": torch.zeros(1000)})
    assert not os.listdir(tmp_path)
