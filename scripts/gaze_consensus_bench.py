#!/usr/bin/env python3
"""The consensus gaze launches timed with device events at the two default multi-view shapes: C3 (I=3, V=4, B=128) and the
per-GPU shape of C5 (I=3, V=8, B=64), inputs of tests/gaze_consensus_ref.py with per-view confidences.  Per shape and per launch
(forward with stats, forward without, backward): --launches back-to-back calls between two events on the current stream after a
warm-up, --repeats times; the figure is the window over the number of launches, i.e. the cost of one more such launch in a
queue that is kept full.  (Each item is one thread walking its D directions in double: the time follows D, not the item count.)
Usage: gaze_consensus_bench.py [--launches N] [--warmup W] [--repeats R] [--out profiles/gaze_consensus.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gaze_consensus_ref as R  # noqa: E402
import rot_mvgaze_amd  # noqa: E402,F401
from rot_mvgaze_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
SHAPES = {"C3": (3, 4, 128), "C5_per_gpu": (3, 8, 64)}


def window_us(fn, launches, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaze_consensus.json"))
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "launches_per_window": a.launches, "warmup": a.warmup, "repeats": a.repeats,
           "how": "torch.cuda.Event pair around back-to-back launches on one stream; microseconds per launch = window / launches",
           "shapes": {}}
    for name, (I, V, B) in SHAPES.items():
        preds, rot = (torch.from_numpy(x).to(dev) for x in R.make_inputs(I, V, B, seed=7))
        w = torch.from_numpy(R.make_weights("confidence", V, B, seed=7)).to(dev)
        mk = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        head, views, stats, dpreds = mk(I, B, 3), mk(I, V, B, 2), mk(I, B, 2), torch.empty_like(preds)
        dviews = torch.from_numpy(np.random.default_rng(11).normal(size=(I, V, B, 2)).astype(np.float32)).to(dev)
        fns = {"fwd_stats": lambda: ops.gaze_consensus_fwd(preds, rot, w, I, V, B, head, views, stats),
               "fwd": lambda: ops.gaze_consensus_fwd(preds, rot, w, I, V, B, head, views, None),
               "bwd": lambda: ops.gaze_consensus_bwd(dviews, preds, rot, w, I, V, B, dpreds)}
        res = {}
        for k, fn in fns.items():
            runs = [round(window_us(fn, a.launches, a.warmup), 3) for _ in range(a.repeats)]
            res[k] = {"us_per_launch_median": statistics.median(runs), "runs": runs}
        out["shapes"][name] = {"iters": I, "views": V, "batch": B, "items": I * B, **res}
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
