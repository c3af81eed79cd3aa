#!/usr/bin/env python
"""One sha256 per case of tests/test_backbone_trace_gpu.py over what the case's step computes, byte for byte: the loss, the
outputs, every parameter gradient in parameter order (and the image gradients where they are asked for) and every buffer -
the BatchNorm running statistics - after the step; for the inference cases the outputs and the activation range record.
The step is deterministic run to run, so two commits that compute the same thing print the same lines:
    python scripts/step_digest.py > a.txt        (on each commit; then diff)
The cases of tests/test_head_trace_gpu.py follow (the fusion head alone): per step the features, predictions and d / d img_feat,
then every head parameter gradient as the last backward left it in the model's gradient views, and the IntensityBatchNorm
running buffers.
Not a test: the digests belong to one ROCm build and one device."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import test_backbone_trace_gpu as T  # noqa: E402
import test_head_trace_gpu as TH  # noqa: E402


def _adder(h):
    def add(tag, t):
        h.update(tag.encode())
        if t is not None:
            h.update(str(tuple(t.shape)).encode() + str(t.dtype).encode())
            h.update(t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy().tobytes())
    return add


def digest(name):
    m, out, loss = T.run_case(name)
    h = hashlib.sha256()
    add = _adder(h)
    add("loss", loss)
    for k in ("img_feat_0", "img_feat_1", "initial_rot_feat_0", "initial_rot_feat_1", "pred_gaze", "_mvg_preds"):
        add(k, out[k])
    for i in range(out["num_iter"]):
        for k in ("feat_0", "feat_1", "pred_gaze_0", "pred_gaze_1"):
            add(f"iter_{i}.{k}", out[f"iter_{i}"][k])
    if loss is not None:
        for k, p in m.named_parameters():
            add("grad " + k, p.grad)
        for k in ("img_0", "img_1"):
            add("grad " + k, out[k].grad if out[k].is_floating_point() else None)
    for k, b in m.named_buffers():
        add("buffer " + k, b)
    add("range", m._backbone._range_record if loss is None else None)
    return h.hexdigest()


def head_digest(name):
    m, results = TH.run_case(name)
    h = hashlib.sha256()
    add = _adder(h)
    for n, r in enumerate(results):
        for k in sorted(r):
            add(f"step{n} {k}", r[k])
    for k, p in m.named_parameters():
        if not k.startswith("_feat_extractor"):
            add("grad " + k, m._grad_views[id(p)] if p.grad is not None else None)
    for k, b in m.named_buffers():
        if not k.startswith("_feat_extractor"):
            add("buffer " + k, b)
    return h.hexdigest()


if __name__ == "__main__":
    for case in sorted(T.CASES):
        print(case, digest(case), flush=True)
    for case in sorted(TH.CASES):
        print("head_" + case, head_digest(case), flush=True)
