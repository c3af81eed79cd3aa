"""A whole training step - zero_grad, forward, loss, backward, fused Adam - captured ONCE in a hipGraph and replayed.

Why: a ResNet-50 step is ~600 kernel launches that the Python host queues one by one through ctypes (~35 us each):
21.5 ms of host time against a 25 ms GPU step at BASELINE config C4's per-GPU share (profiles/r03_bench_c4.json), i.e.
the data-parallel configurations sit at the edge of being host-bound.  Nothing on the step path synchronises or
depends on host data (tests/test_model_gpu.py::test_training_step_does_not_synchronise_the_host), the optimizer's step
counter and learning rate live on the device (optim.Adam(capturable=True)), and the side stream of the weight-gradient
kernels forks from / joins the capturing stream through events - so the step is capturable as it stands; a replay costs
the host one hipGraphLaunch.  (The reference's caller: /root/reference/trainer.py:119-147 - model(data), metrics(data),
zero_grad, backward, optimizer.step per iteration.)

Measured on MI355X / ROCm 7.0 (scripts/graph_probe.py, profiles/README.md round 4): a replay costs the host 0.08-0.15 ms
instead of 5-20 ms, and takes exactly the GPU time of the eager step WITHOUT the side stream (C4's share 27.98 vs 27.80 ms,
C2 9.73 vs 9.74): the eager step is GPU-bound, so the graph buys host time, not throughput.  A capture that includes the
weight-gradient side stream (fork / join events -> a branching graph) replays 1.45-1.7x SLOWER than the eager step (38.0 vs
26.2 ms, 15.3 vs 9.0): the capture is therefore taken single-stream (overlap_wgrad off), which gives up the ~6 % the
overlap is worth on one GPU.  Use it where the host is the bottleneck (many ranks per host, small per-GPU batches).

Fine-tuning steps (frozen parameters, parameter groups, model.freeze_batchnorm) capture the same way over
optim.Adam(capturable="segments"): one learning rate per group and one step counter per segment on the device.  The captured
launches hold that optimizer's plan by value, so run() checks on the host that the plan is still the captured one and raises
otherwise (scripts/graph_finetune_bench.py, profiles/r20_graph_finetune_bench.json: ResNet-50 V=4 B=32 with the stem, layer1 and
layer2 frozen replays at 16.8 ms of GPU time and 0.16 ms of host time against 15.95 / 13.2 ms eager with the side stream).

PyTorch here is plumbing only: ``torch.cuda.CUDAGraph`` is hipStreamBeginCapture / hipGraphInstantiate / hipGraphLaunch
plus a private pool of the caching allocator, which is what keeps every buffer the captured launches point at alive
and un-recycled between replays.
"""
from __future__ import annotations

from typing import Callable, List, Optional

import torch

Tensor = torch.Tensor


class GraphedStep:
    """``step_fn()`` -> loss: one training step on STATIC input tensors (the caller refills them in place between
    replays: ``img.copy_(next_batch)``).  ``run()`` replays the captured step and returns the (static) loss tensor."""

    def __init__(self, model, step_fn: Callable[[], Tensor], optimizer=None, warmup: int = 3):
        if optimizer is not None and not getattr(optimizer, "capturable", False):
            raise ValueError("GraphedStep needs rot_mvgaze_amd.optim.Adam(capturable=True): the step counter and the "
                             "learning rate must live on the device")
        aug = getattr(model, "input_augment", None)
        if aug is not None and not getattr(aug, "capturable", False):     # TrainAugment(draws="device") draws in a launch of its own
            raise RuntimeError("GraphedStep: model.input_augment draws on the host for every step and cannot be captured: augment "
                               "outside the step (TrainAugment.apply into the static input) and set input_augment = None")
        self.model, self.optimizer = model, optimizer
        self._step_fn = step_fn
        dev = next(model.parameters()).device
        model.ensure_layout()
        model._backbone.overlap_wgrad = False          # single-stream capture (see the module docstring)
        # eager warm-up on a side stream (allocator pools, weight-copy tables, scratch registration, the optimizer's
        # device state): capture must find nothing left to set up
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            for _ in range(max(1, warmup)):
                step_fn()
        torch.cuda.current_stream(dev).wait_stream(s)
        torch.cuda.synchronize(dev)
        if optimizer is not None:
            optimizer.sync_lr()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss = step_fn()
        self.replays = 0
        # capturable="segments": the captured launches hold the optimizer's plan (which ranges are updated, from which group, with
        # which constants) and point at its device table; what they were captured for is checked before every replay
        self._plan = self._plan_now() if getattr(optimizer, "capturable", None) == "segments" else None
        self._arena_params = [p for (p, _, _) in model.grad_arena()[1]] if self._plan is not None else None

    def _plan_now(self):
        return (self.optimizer.plan_signature(), [p.requires_grad for (p, _, _) in self.model.grad_arena()[1]], self.optimizer.plan_epoch(),
                self.optimizer.plan_inputs())

    def _check_plan(self) -> None:
        """Host-only: a replay would go on updating a now-frozen parameter from its stale gradient (and never touch an unfrozen one)."""
        # the signature is a function of the flags, the groups' constants and sizes and the table's epoch: nothing to plan while
        # those are what they were (the common replay)
        if self._plan[1] == [p.requires_grad for p in self._arena_params] and self._plan[3] == self.optimizer.plan_inputs():
            return
        sig, flags, epoch, inputs = self._plan_now()
        if flags != self._plan[1]:
            names = {id(p): k for k, p in self.model.named_parameters()}
            moved = [names.get(id(p), "?") for (p, _, _), a, b in zip(self.model.grad_arena()[1], self._plan[1], flags) if a != b]
            what = f"requires_grad of {len(moved)} parameter(s) changed since the capture (first: {moved[0]})"
        elif sig != self._plan[0]:
            what = "the optimizer's plan changed since the capture (parameter groups, betas, eps, weight_decay or decoupled_weight_decay)"
        elif epoch != self._plan[2]:
            what = "the optimizer rebuilt its device state since the capture (an eager step with another plan ran in between)"
        elif inputs[2:] != self._plan[3][2:]:
            what = "the optimizer's max_grad_norm or skip_nonfinite changed since the capture (both travel by value in the captured launches)"
        else:
            return
        raise RuntimeError(f"GraphedStep: {what}; the captured step no longer matches - run one eager step and build a new GraphedStep")

    def run(self) -> Tensor:
        if self._plan is not None:
            self._check_plan()
        if self.optimizer is not None:
            self.optimizer.sync_lr()                 # a scheduler may have moved the learning rate: one 4-byte fill
        self.graph.replay()
        self.replays += 1
        # the captured kernels rewrote the parameters through raw pointers: drop the inference path's cached weight copies
        self.model.invalidate_weight_cache()
        return self.loss
