#!/usr/bin/env python3
"""What the inference range guard costs (Backbone.split_eval_guard): the eval-mode forward of BASELINE
configs C3 (ResNet-50, V = 4, B = 128) and C2 (ResNet-18, V = 2, B = 64) at 224 px under torch.no_grad(), with the guard in
each setting - None, "record", "fallback" - run in ALTERNATION in one process on one box: ROUNDS rounds, each timing CALLS
forwards per setting with device events.  Per setting: the median and minimum over all calls and the per-round medians; the
unguarded path's own round-to-round spread (largest minus smallest round median) is the yardstick a difference has to beat.
Then the largest conv launches of C3's forward, mvg_conv_fprop_split_affine against mvg_conv_fprop_split_affine_ranged on the
same operands, alternating too.  Synthetic weights and inputs (a clean checkpoint: "fallback" never reruns).
Usage: range_guard_bench.py [--rounds R] [--calls N] [--warmup W] [--out FILE.json] [--small]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import rot_mvgaze_amd  # noqa: E402,F401
from rot_mvgaze_amd import ops, synth  # noqa: E402
from rot_mvgaze_amd._lib import ConvDesc  # noqa: E402
from rot_mvgaze_amd.geometry import rotation_matrix_2d  # noqa: E402
from rot_mvgaze_amd.model import MultiViewGaze  # noqa: E402

dev = torch.device("cuda:0")
GUARDS = (None, "record", "fallback")
CONFIGS = [("C3 eval: R50 V=4 B=128 224px", 50, 4, 128, 224), ("C2 eval: R18 V=2 B=64 224px", 18, 2, 64, 224)]
# C3's largest forward conv launches (G, N, h, cin, cout, k, stride, pad): the most workgroups (64 -> 256 at 56 x 56: 25 088 tiles of
# 128 x 128), the 256 x 64 tile's (64 -> 64 3x3 at 56 x 56), and the most output bytes per flop at the next stage (128 -> 512 at 28 x 28)
LAUNCHES = [(4, 128, 56, 64, 256, 1, 1, 0), (4, 128, 56, 64, 64, 3, 1, 1), (4, 128, 28, 128, 512, 1, 1, 0)]


def timed(fn, calls):
    ts = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def summary(per_round):
    flat = [t for r in per_round for t in r]
    meds = [float(np.median(r)) for r in per_round]
    return {"ms_median": round(float(np.median(flat)), 4), "ms_min": round(float(np.min(flat)), 4),
            "round_medians_ms": [round(m, 4) for m in meds], "round_spread_ms": round(max(meds) - min(meds), 4)}


def alternate(fns, rounds, calls, warmup):
    """fns: {name: callable}.  Warm every one up, then ROUNDS times: each in turn, CALLS timed calls."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    per = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            per[k].append(timed(fn, calls))
    return {k: summary(v) for k, v in per.items()}


def model_config(depth, V, B, hw, rounds, calls, warmup):
    m = MultiViewGaze(depth, 3)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.make_state_dict(depth, 0, 3).items()})
    m.to(dev).eval()
    m.ensure_layout()
    assert m._backbone.split and m._backbone.split_eval
    inp = synth.make_inputs(B, V, 1234, hw)
    img = [torch.from_numpy(inp["img"][:, v]).contiguous().to(dev) for v in range(V)]
    rot = rotation_matrix_2d(torch.from_numpy(inp["head_pose"]).reshape(-1, 2).to(dev)).reshape(B, V, 3, 3).contiguous()

    def forward(guard):
        def run():
            m.split_eval_guard = guard
            with torch.no_grad():
                return m.run_views(img, rot)
        return run
    ref = [o.clone() for o in forward(None)()]
    for g in GUARDS[1:]:                                   # faster and different is not faster
        assert all(torch.equal(a, b) for a, b in zip(forward(g)(), ref)), g
        assert m.overflowed() == []
    res = alternate({str(g): forward(g) for g in GUARDS}, rounds, calls, warmup)
    m.split_eval_guard = "record"
    forward("record")()
    rep = m.range_report()
    top = max(rep, key=rep.get)
    base = res["None"]["ms_median"]
    for g in ("record", "fallback"):
        res[g]["minus_unguarded_ms"] = round(res[g]["ms_median"] - base, 4)
        res[g]["over_unguarded"] = round(res[g]["ms_median"] / base, 5)
    res["unguarded_round_spread_ms"] = res["None"]["round_spread_ms"]
    res["largest_activation"] = {"unit": top, "value": rep[top]}
    m.split_eval_guard = None
    return res


def launch_case(case, rounds, calls, warmup):
    G, N, h, cin, cout, k, st, pad = case
    d = ConvDesc.make(G, N, h, h, cin, cout, k, st, pad)
    torch.manual_seed(0)
    xs = ops.split_f32(torch.relu(torch.randn(G, N, h, h, cin, device=dev)))
    wk, _ = ops.split_weights(d, torch.randn(cout, k, k, cin, device=dev) * (1.0 / (k * k * cin) ** 0.5), False)
    scale, shift = torch.rand(cout, device=dev) + 0.5, torch.randn(cout, device=dev) * 0.5
    out = ops.sp_empty(G, N, d.ho, d.wo, cout, device=dev)
    out2 = ops.sp_empty(G, N, d.ho, d.wo, cout, device=dev)
    word = torch.zeros(1, dtype=torch.int32, device=dev)

    def unranged():
        ops.conv_fprop_split_affine(d, xs, wk, out, scale, shift, None, True)

    def ranged():                                          # (the word keeps its value between calls: the steady state of one forward -
        ops.conv_fprop_split_affine_ranged(d, xs, wk, out2, scale, shift, None, True, word)     # few atomics; "cold" below clears it)

    def ranged_cold():
        word.zero_()
        ops.conv_fprop_split_affine_ranged(d, xs, wk, out2, scale, shift, None, True, word)
    res = alternate({"unranged": unranged, "ranged": ranged, "ranged_cleared_word": ranged_cold}, rounds, calls, warmup)
    assert torch.equal(out.view(torch.int16), out2.view(torch.int16))
    tiles = G * -(-(N * d.ho * d.wo) // (256 if (cout < 128 and k > 1 and N * d.ho * d.wo >= 65536) else 128)) * -(-cout // (128 if cout >= 128 else 64))
    res["workgroups"] = tiles
    res["ranged_over_unranged"] = round(res["ranged"]["ms_median"] / res["unranged"]["ms_median"], 5)
    res["ranged_cleared_over_unranged"] = round(res["ranged_cleared_word"]["ms_median"] / res["unranged"]["ms_median"], 5)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_range_guard.json"))
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes (numbers mean nothing)")
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "calls_per_round": a.calls, "warmup": a.warmup,
           "timing": "device events around one forward / one launch; settings alternate inside every round", "forward": {}, "launches": {}}
    configs = [("toy: R18 V=2 B=2 64px", 18, 2, 2, 64)] if a.small else CONFIGS
    launches = [(1, 2, 16, 64, 128, 1, 1, 0)] if a.small else LAUNCHES
    for name, depth, V, B, hw in configs:
        out["forward"][name] = model_config(depth, V, B, hw, a.rounds, a.calls, a.warmup)
        print(name, json.dumps(out["forward"][name]), flush=True)
        torch.cuda.empty_cache()
    for case in launches:
        name = "g%d n%d %dx%d %d->%d k%d s%d" % (case[0], case[1], case[2], case[2], case[3], case[4], case[5], case[6])
        out["launches"][name] = launch_case(case, a.rounds, 2 * a.calls, a.warmup)
        print(name, json.dumps(out["launches"][name]), flush=True)
        torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
