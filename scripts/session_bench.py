#!/usr/bin/env python3
"""Inference session against the Python no_grad path: host time to queue one forward, and GPU time per forward.

Same box, same process, Python path first then the session, both after warm-up, per shape (ResNet-50, 224 px):
(V2, B1), (V4, B8) and the C3 eval shape (V4, B128) - each once for the fp32 model and once for the bf16 inference form
(compute_dtype = torch.bfloat16 against InferenceSession(..., compute=torch.bfloat16); the Python path's bf16 weight copies are
warm too: its warm-up calls made them and nothing invalidates them).  Per path:
  host_ms   median over >= 50 calls of perf_counter around ONE call, the stream idle before it and no sync inside;
  gpu_ms    hipEvents around a back-to-back run of calls, divided by their number (a host-bound path shows its host time here);
  launches  library launches of one forward counted by the profiler (mvg_prof_collect); the session also reports
            mvg_session_launches (its plan's step count; mvg_absmax_multi and the slot clear carry no profiler scope).
The Python path re-queues its per-call weight work every call (one bn_eval_affine per conv; on the split head path a re-split
of the fuser / head weights); the session queues neither after bind.  The two paths' outputs are compared (torch.equal) first.

Each shape runs in a child process of its own under its own time limit; the parent stops at the first child that does not
exit cleanly.  One JSON line per (shape, compute form) goes to --out (default profiles/r11_session_bench.json).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(2, 1), (4, 8), (4, 128)]
DEPTH, HW, ITERS = 50, 224, 3


def run_case(V, B, calls, reps, compute="fp32"):
    import numpy as np
    import torch
    import rot_mvgaze_amd  # noqa: F401
    from rot_mvgaze_amd import ops, synth
    from rot_mvgaze_amd.geometry import rotation_matrix_2d
    from rot_mvgaze_amd.model import FeatRotationSymm
    from rot_mvgaze_amd.session import InferenceSession
    dev = torch.device("cuda:0")
    m = FeatRotationSymm(DEPTH, ITERS)
    sd = synth.make_state_dict(DEPTH, 0, ITERS, perturb_bn=True)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    m.to(dev).eval()
    bf16 = compute == "bf16"
    if bf16:
        m.compute_dtype = torch.bfloat16
    inp = synth.make_inputs(B, V, 1234, HW)
    imgs = [torch.from_numpy(np.ascontiguousarray(inp["img"][:, v])).to(dev) for v in range(V)]
    rot = rotation_matrix_2d(torch.from_numpy(inp["head_pose"]).reshape(-1, 2).to(dev)).reshape(B, V, 3, 3).contiguous()
    sess = InferenceSession(m, V, B, HW, HW, compute=torch.bfloat16 if bf16 else None)
    out = sess.empty_outputs()

    def python_path():
        with torch.no_grad():
            return m.run_views(imgs, rot)

    def session_path():
        return sess.run(imgs, rot, out=out)

    want = [o.clone() for o in python_path()]
    got = session_path()
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in zip(got, want))

    def measure(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        host = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            host.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
        gpu = []
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            gpu.append(a.elapsed_time(b) / reps)
        ops.prof_reset()
        ops.prof_enable(True)
        try:
            fn()
            torch.cuda.synchronize()
            prof = ops.prof_collect()
        finally:
            ops.prof_enable(False)
        return {"host_ms": round(1e3 * statistics.median(host), 4), "host_ms_min": round(1e3 * min(host), 4),
                "gpu_ms": round(statistics.median(gpu), 4), "gpu_ms_runs": [round(g, 4) for g in gpu],
                "launches": int(sum(e["launches"] for e in prof.values())),
                "kernel_ms": round(sum(e["ms"] for e in prof.values()), 4)}

    rec = {"shape": {"depth": DEPTH, "views": V, "batch": B, "hw": HW, "num_iter": ITERS}, "compute": compute,
           "device": torch.cuda.get_device_name(0),
           "calls": calls, "bit_identical": bool(same), "python": measure(python_path), "session": measure(session_path)}
    rec["session"]["plan_launches"] = sess.launches
    rec["session"]["workspace_bytes"] = sess.workspace_bytes
    rec["backbone_split"] = bool(m._backbone._split_now) and not bf16
    rec["head_rows"] = V * (V - 1) * B
    sess.close()
    print("SESSION_BENCH " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", nargs=2, type=int, metavar=("V", "B"), help="run one shape in this process")
    ap.add_argument("--compute", choices=("fp32", "bf16"), default="fp32", help="with --case: the compute form of both paths")
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_session_bench.json"))
    a = ap.parse_args()
    if a.case:
        run_case(a.case[0], a.case[1], max(a.calls, 50), a.reps, a.compute)
        return 0
    lines = []
    cases = [(V, B, compute) for compute in ("fp32", "bf16") for V, B in SHAPES]
    for V, B, compute in cases:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", str(V), str(B), "--compute", compute, "--calls", str(a.calls),
               "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(f"V{V} B{B} {compute}: no result within {a.timeout} s - stopping here", file=sys.stderr)
            break
        rec = [ln[len("SESSION_BENCH "):] for ln in r.stdout.splitlines() if ln.startswith("SESSION_BENCH ")]
        if r.returncode != 0 or not rec:
            print(f"V{V} B{B} {compute}: exit code {r.returncode} - stopping here\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            break
        lines.append(rec[-1])
        print(rec[-1], flush=True)
    if lines:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if len(lines) == len(cases) else 1


if __name__ == "__main__":
    sys.exit(main())
