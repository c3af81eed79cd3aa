#!/usr/bin/env python
"""One sha256 per case of tests/test_backbone_trace_gpu.py over what the case's step computes, byte for byte: the loss, the
outputs, every parameter gradient in parameter order (and the image gradients where they are asked for) and every buffer -
the BatchNorm running statistics - after the step; for the inference cases the outputs and the activation range record.
The step is deterministic run to run, so two commits that compute the same thing print the same lines:
    python scripts/step_digest.py > a.txt        (on each commit; then diff)
Not a test: the digests belong to one ROCm build and one device."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import test_backbone_trace_gpu as T  # noqa: E402


def digest(name):
    m, out, loss = T.run_case(name)
    h = hashlib.sha256()

    def add(tag, t):
        h.update(tag.encode())
        if t is not None:
            h.update(str(tuple(t.shape)).encode() + str(t.dtype).encode())
            h.update(t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy().tobytes())
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


if __name__ == "__main__":
    for case in sorted(T.CASES):
        print(case, digest(case), flush=True)
