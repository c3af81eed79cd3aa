"""Adam with the reference trainer's configuration surface, one fused HIP launch per step.

Mirrors ``optim.Adam(self.model.parameters(), lr=0, weight_decay=1e-6)`` of
/root/reference/trainer.py:54 (stepped at :141-143, lr driven by CyclicLR :58-62): a
``torch.optim.Optimizer`` subclass, so ``CyclicLR(optimizer, ..., cycle_momentum=False)`` works on it
unchanged.  The update itself is ``mvg_adam_step`` over the model's parameter / gradient arenas
(identical offsets), i.e. one kernel for all ~90 M parameters instead of ~190 foreach launches.

Fine-tuning goes beyond the reference's one group: any number of parameter groups, each with its own ``lr`` / ``betas`` /
``eps`` / ``weight_decay``, and parameters without a gradient (frozen ones, ``requires_grad = False``) skipped as torch skips
them - value, moments and step count untouched.  Step counts are per parameter (``torch.optim.Adam``'s ``state[p]['step']``):
a parameter unfrozen at step 5 starts its bias correction at 1.  Such a step is ``mvg_adam_step_segments``: ``plan_segments``
merges arena-adjacent parameters with a gradient, the same hyper-parameters and the same step count into element ranges, and
one launch (16 ranges at a time) updates those ranges only.  One group with every gradient present and one step count is the
reference-shaped case and stays the ``mvg_adam_step`` launch.

``capturable="segments"`` is that fine-tuning step for a hipGraph (graph.GraphedStep): ``mvg_adam_step_segments_dev`` takes the
segments' bounds and constants by value, as above, but reads each group's learning rate from a device vector and each segment's
step count and bias corrections from a device table that the step itself advances - a replay needs nothing from the host.  The
segments, their group indices and constants are the PLAN; its signature tells when the table has to be rebuilt (a parameter was
frozen or unfrozen, a group added, betas changed), which happens in an eager step only, from the counts read back from the device.

``max_grad_norm`` / ``skip_nonfinite`` add global-norm gradient clipping and a guard against non-finite gradients to the step
itself.  One read of the gradients of the parameters that take part (``mvg_grad_norm_segments`` over the plan's segments) leaves
``{norm, coef, skipped, skipped_total}`` on the device; the segmented update multiplies each gradient by ``coef`` as it loads it
and, like the tick of the device-resident counters, returns at once when ``skipped`` is set.  Two differences from
``torch.nn.utils.clip_grad_norm_``: ``.grad`` KEEPS THE UNSCALED GRADIENT (nothing rewrites the gradient arena; the scaled value
exists only inside the update), and the norm counts exactly the parameters that take part in the step - a frozen or group-less
parameter's stale ``.grad`` is not in it.  Clipping alone adds no synchronisation.  ``skip_nonfinite`` with ``capturable=False``
reads the 16-byte record back after the norm launches - the ONE synchronisation this mode adds (``GradScaler.step`` does the
same) - and on a skip launches no update and leaves the host step counts alone; with ``capturable="segments"`` nothing comes
back to the host: the tick and the update read ``skipped`` on the device, so a captured replay clips and skips by itself.

``decoupled_weight_decay`` (a default and a per-group key, ``torch.optim.Adam``'s name; ``AdamW`` is ``Adam`` with it set and
``weight_decay=1e-2``) selects ``torch.optim.AdamW``'s decay inside the same launches: the parameter is shrunk by
``1 - lr * weight_decay`` and the moments see the gradient alone.  The mode is one more by-value constant of a segment - it is in
``_hyper`` and ``_segment_key``, so neighbours that differ in it never share a segment, and flipping it changes the plan.  The
reference-shaped step is ``mvg_adamw_step`` / ``mvg_adamw_step_dev``; every segmented path calls the ``_ex`` entry points (a mode
per segment, coupled and decoupled groups in one launch) as soon as one group is decoupled, and exactly today's entry points
while none is.  A checkpoint written before the key existed loads with ``decoupled_weight_decay = False`` in every group.
"""
from __future__ import annotations

from typing import Dict, Hashable, List, NamedTuple, Sequence, Tuple

import torch

from . import ops


class Segment(NamedTuple):
    """One element range [begin, end) of the arenas (both multiples of 4) updated with one set of hyper-parameters."""
    begin: int
    end: int
    group: Hashable       # what plan_segments was given as the parameters' group key
    step: int


def plan_segments(entries: Sequence[Tuple[int, int]], group_of: Sequence[Hashable], has_grad: Sequence[bool],
                  steps: Sequence[int]) -> List[Segment]:
    """The segments of one optimizer step, from the arena layout alone (no device, no library).

    entries: (offset, numel) of every arena parameter, in arena order (offsets are multiples of 4: every entry starts on a
    16-byte slot); group_of[i]: a hashable key - two parameters may share a segment only when their keys are equal (optim.Adam
    passes the group's hyper-parameters); has_grad[i]: whether parameter i takes part in this step; steps[i]: the step count
    this update uses for it (>= 1, i.e. already advanced).

    Maximal runs of arena-adjacent parameters that take part and agree in key and step count become one segment.  Bounds are
    rounded to the 4-element slots: a run ends on its last entry's slot boundary, so the zero padding between and behind
    entries (2-element head biases) sits inside the run - Adam maps zero parameter, gradient and moments to zero.  Sorted by
    begin, disjoint."""
    if not (len(entries) == len(group_of) == len(has_grad) == len(steps)):
        raise ValueError("plan_segments: entries, group_of, has_grad and steps must have one item per parameter")
    out: List[Segment] = []
    cur = None                                    # [begin, end, key, step] of the open run
    last_end = 0
    for (off, numel), key, has, step in zip(entries, group_of, has_grad, steps):
        if off % 4 or numel <= 0 or off < last_end:
            raise ValueError(f"plan_segments: entry at {off} (+{numel}) is unaligned, empty or out of arena order")
        end = last_end = (off + numel + 3) // 4 * 4
        if not has:
            if cur is not None:
                out.append(Segment(*cur))
                cur = None
            continue
        if step < 1:
            raise ValueError("plan_segments: a parameter that takes part needs a step count >= 1")
        if cur is not None and cur[1] == off and cur[2] == key and cur[3] == step:
            cur[1] = end
            continue
        if cur is not None:
            out.append(Segment(*cur))
        cur = [off, end, key, int(step)]
    if cur is not None:
        out.append(Segment(*cur))
    return out


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, capturable=False, max_grad_norm=None,
                 skip_nonfinite=False, decoupled_weight_decay=False):
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("invalid Adam hyper-parameter")
        # decoupled_weight_decay (torch.optim.Adam's name for it; a group may override it): False is Adam's coupled L2 decay,
        # g + wd * p in both moments; True is AdamW's, p shrunk by 1 - lr * wd and the moments from the gradient alone.  Every
        # group carries the key (add_param_group fills it in); ``defaults`` keeps the four keys it always had.
        self._decoupled_default = bool(decoupled_weight_decay)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        for g in self.param_groups:
            if g["lr"] < 0 or g["eps"] < 0 or g["weight_decay"] < 0 or not (0 <= g["betas"][0] < 1 and 0 <= g["betas"][1] < 1):
                raise ValueError("invalid Adam hyper-parameter in a parameter group")
        self._flat: Dict[int, dict] = {}
        self._pending = None          # moments restored by load_state_dict, adopted by the next step()
        # capturable (like torch.optim.Adam's flag): the step counter, the bias corrections and the learning rate live on
        # the DEVICE (mvg_adam_step_dev), so that a step captured in a hipGraph (rot_mvgaze_amd.graph.GraphedStep) replays
        # with nothing from the host; the learning rate is pushed to the device by sync_lr() - outside a capture - whenever
        # the scheduler changed it (the reference steps CyclicLR once per epoch, trainer.py:147).
        # capturable="segments": the same for the fine-tuning step - any number of groups, parameters without a gradient skipped,
        # per-parameter step counts (mvg_adam_step_segments_dev: one learning rate per group and one counter per segment on the
        # device).  Opt-in: True keeps meaning exactly the one-group, nothing-skipped step.
        if isinstance(capturable, str) and capturable != "segments":
            raise ValueError(f"Adam: capturable must be False, True or 'segments', not {capturable!r}")
        self.capturable = "segments" if isinstance(capturable, str) else bool(capturable)
        if self.capturable is True and len(self.param_groups) != 1:
            raise NotImplementedError("Adam(capturable=True) takes one parameter group (refused at construction): the captured "
                                      "step keeps ONE learning rate and ONE step counter on the device; grouped steps run with "
                                      "capturable=False")
        # max_grad_norm (None: no clipping) / skip_nonfinite: attributes of the optimizer, not of its groups - the norm is global,
        # and state_dict() keeps the keys it had (see the module docstring for what they do and what they cost)
        self._check_max_grad_norm(max_grad_norm)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        if self.capturable is True and self._clipping():
            raise ValueError("Adam(capturable=True) takes neither max_grad_norm nor skip_nonfinite: clipping and the guard run on the "
                             "segmented step; use capturable='segments' (it serves one parameter group as well)")

    def add_param_group(self, param_group):
        """torch's, with the optimizer's decay mode as the default of a group that names none."""
        if isinstance(param_group, dict):
            param_group.setdefault("decoupled_weight_decay", self._decoupled_default)
            param_group["decoupled_weight_decay"] = bool(param_group["decoupled_weight_decay"])
        super().add_param_group(param_group)

    @staticmethod
    def _check_max_grad_norm(value) -> None:
        if value is not None and not float(value) > 0:
            raise ValueError(f"Adam: max_grad_norm must be None or > 0, not {value!r}")

    def _clipping(self) -> bool:
        return self.max_grad_norm is not None or bool(self.skip_nonfinite)

    def sync_lr(self):
        """capturable: copy param_groups[0]['lr'] to the device scalar the captured update reads (no-op when unchanged);
        capturable="segments": every group's learning rate that changed, to its slot of the device vector."""
        if self.capturable == "segments":
            lrs = [float(g["lr"]) for g in self.param_groups]
            for st in self._flat.values():
                if "lr_dev" not in st:
                    continue
                for i in range(min(len(lrs), len(st["lr_host"]))):
                    if st["lr_host"][i] != lrs[i]:
                        if torch.cuda.is_current_stream_capturing():
                            raise RuntimeError("Adam(capturable='segments'): a learning rate changed inside a graph capture; call "
                                               "optimizer.sync_lr() before capturing / replaying")
                        st["lr_dev"][i:i + 1].fill_(lrs[i])
                        st["lr_host"][i] = lrs[i]
            return
        lr = float(self.param_groups[0]["lr"])
        for st in self._flat.values():
            if "lr_dev" in st and st["lr_host"] != lr:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("Adam(capturable=True): the learning rate changed inside a graph capture; call "
                                       "optimizer.sync_lr() before capturing / replaying")
                st["lr_dev"].fill_(lr)
                st["lr_host"] = lr

    def _owners(self):
        owners = {}
        for g in self.param_groups:
            for p in g["params"]:
                ref = getattr(p, "_mvg_owner", None)
                model = ref() if ref is not None else None
                if model is None:
                    raise RuntimeError("rot_mvgaze_amd.optim.Adam only updates parameters of the MI355X "
                                       "FeatRotationSymm / MultiViewGaze modules")
                owners[id(model)] = model
        return list(owners.values())

    @staticmethod
    def _hyper(g) -> tuple:
        return (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]),
                int(bool(g["decoupled_weight_decay"])))       # the mode: 0 coupled, 1 decoupled, as the C ABI takes it

    def _any_decoupled(self) -> bool:
        return any(bool(g["decoupled_weight_decay"]) for g in self.param_groups)

    def _step_segments_host(self, arena_p, arena_g, st, segs: Sequence[Segment], clip4) -> None:
        """The host-lr segmented update over ``segs`` (keys from _hyper): today's entry points while no group is decoupled, the
        _ex one - a mode per segment - as soon as one is."""
        if self._any_decoupled():
            ops.adam_step_segments_ex(arena_p, arena_g, st["exp_avg"], st["exp_avg_sq"],
                                      [(s.begin, s.end) + s.group[:5] + (s.step, s.group[5]) for s in segs], clip4)
            return
        records = [(s.begin, s.end) + s.group[:5] + (s.step,) for s in segs]
        if clip4 is None:
            ops.adam_step_segments(arena_p, arena_g, st["exp_avg"], st["exp_avg_sq"], records)
        else:
            ops.adam_step_segments_clip(arena_p, arena_g, st["exp_avg"], st["exp_avg_sq"], records, clip4)

    def _state_for(self, model, arena_p, n_entries: int) -> dict:
        """The flat state of ``model``: the two moment buffers at arena offsets and one step count per arena parameter."""
        st = self._flat.get(id(model))
        if st is None and self._pending:
            saved = self._pending.pop(0)
            if saved["exp_avg"].numel() != arena_p.numel():
                raise RuntimeError("optimizer state does not match this model's parameter arena "
                                   f"({saved['exp_avg'].numel()} vs {arena_p.numel()} elements)")
            # (an entry written before per-parameter counts existed holds one "step": every parameter gets it)
            steps = [int(s) for s in saved["steps"]] if "steps" in saved else [int(saved["step"])] * n_entries
            if len(steps) != n_entries:
                raise RuntimeError(f"optimizer state holds {len(steps)} step counts for {n_entries} arena parameters")
            st = {"step": max(steps), "steps": steps, "n": arena_p.numel(),
                  "exp_avg": saved["exp_avg"].to(arena_p.device, torch.float32).contiguous(),
                  "exp_avg_sq": saved["exp_avg_sq"].to(arena_p.device, torch.float32).contiguous()}
            self._flat[id(model)] = st
        if st is None or st["exp_avg"].data_ptr() == 0 or st["n"] != arena_p.numel() or \
                st["exp_avg"].device != arena_p.device or len(st["steps"]) != n_entries:
            st = {"step": 0, "steps": [0] * n_entries, "n": arena_p.numel(), "exp_avg": torch.zeros_like(arena_p),
                  "exp_avg_sq": torch.zeros_like(arena_p)}
            self._flat[id(model)] = st
        return st

    # ---- capturable="segments": the plan, its signature and the device table
    @staticmethod
    def _segment_key(index: int, g) -> tuple:
        """What two parameters must share to share a segment of the device-resident step: the group (its INDEX - two groups with
        equal learning rates today may differ tomorrow) and the constants that travel by value, the decay mode among them.  The
        learning rate is not in it."""
        return (index, float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]),
                int(bool(g["decoupled_weight_decay"])))

    def _plan(self, entries, have, steps) -> List[Segment]:
        """plan_segments over ``entries`` = [(param, offset, numel)] for the parameters ``have`` marks, from counts ``steps`` so far."""
        key_of = {id(p): self._segment_key(i, g) for i, g in enumerate(self.param_groups) for p in g["params"]}
        return plan_segments([(off, n) for (_, off, n) in entries], [key_of.get(id(p)) for (p, _, _) in entries], have,
                             [s + 1 if h else s for s, h in zip(steps, have)])

    @staticmethod
    def _signature(segs: Sequence[Segment]) -> tuple:
        """Bounds, group index and by-value constants per segment.  No step count and no learning rate: every row advances once per
        step, so counts that agreed (or differed) when the table was built still do, and learning rates live in lr_dev."""
        # (a coupled segment's item is what it was before the mode existed; a decoupled one's ends in "decoupled")
        return tuple((s.begin, s.end) + s.group[:5] + (("decoupled",) if s.group[5] else ()) for s in segs)

    def plan_signature(self, entries=None) -> tuple:
        """The signature of the plan the next step would run if every parameter that requires a gradient received one.  Host-only
        (no device read, no launch): graph.GraphedStep compares it before every replay.  ``entries`` = [(param, offset, numel)] in
        arena order; by default the arena of every model the parameters belong to."""
        group_params = {id(p) for g in self.param_groups for p in g["params"]}
        lists = [(None, entries)] if entries is not None else [(m, m.grad_arena()[1]) for m in self._owners()]
        out = []
        for model, ents in lists:
            st = self._flat.get(id(model)) if model is not None else None
            steps = st["steps"] if st is not None and len(st["steps"]) == len(ents) else [0] * len(ents)
            have = [id(p) in group_params and p.requires_grad for (p, _, _) in ents]
            out.append(self._signature(self._plan(ents, have, steps)))
        return tuple(out)

    def plan_inputs(self) -> tuple:
        """What plan_signature() is a function of besides the parameters' requires_grad flags: each group's size and by-value
        constants, and the epoch of the device tables (whose counts decide which neighbours may share a segment); and what else a
        captured step holds by value: max_grad_norm and skip_nonfinite."""
        return (tuple((len(g["params"]),) + self._segment_key(i, g) for i, g in enumerate(self.param_groups)), self.plan_epoch(),
                (None if self.max_grad_norm is None else float(self.max_grad_norm), bool(self.skip_nonfinite)))

    def plan_epoch(self) -> tuple:
        """How often each model's device table was (re)built: a graph captured before a rebuild points at the old table."""
        return tuple(st.get("epoch", 0) for st in self._flat.values())

    @staticmethod
    def _pull_steps(st) -> None:
        """Per-parameter counts from the device table - the truth, since replays advance it without Python (one small copy)."""
        if "state3" in st:
            rows = [int(round(x)) for x in st["state3"][:, 0].cpu().tolist()]
            st["steps"] = [rows[k] if k >= 0 else s for s, k in zip(st["steps"], st["seg_of"])]
            st["step"] = max(st["steps"])

    def _step_segments_dev(self, st, entries, have, arena_p, arena_g) -> None:
        segs = self._plan(entries, have, st["steps"])
        if self._signature(segs) != st.get("sig") or len(st["lr_host"]) != len(self.param_groups):
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("Adam(capturable='segments'): the plan of this step (which parameters hold a gradient, their groups, "
                                   "betas / eps / weight_decay) is not the one its device state was built for; run one eager step "
                                   "before capturing (the device table is created and rebuilt there, never inside a capture)")
            self._pull_steps(st)                       # counts as the device advanced them, then the plan from those
            segs = self._plan(entries, have, st["steps"])
            dev = arena_p.device
            st["sig"] = self._signature(segs)
            st["segs"] = [(s.begin, s.end) + s.group for s in segs]
            st["segs_coupled"] = [r[:7] for r in st["segs"]]
            st["seg_of"] = [next((k for k, s in enumerate(segs) if s.begin <= off < s.end), -1) if h else -1
                            for (_, off, _), h in zip(entries, have)]
            # a row holds the count so far; the step's own launch advances it (a parameter unfrozen later starts at step 1)
            st["state3"] = torch.tensor([[float(s.step - 1), 0.0, 0.0] for s in segs], dtype=torch.float32).reshape(-1, 3).to(dev)
            st["lr_host"] = [float(g["lr"]) for g in self.param_groups]
            st["lr_dev"] = torch.tensor(st["lr_host"], dtype=torch.float32).to(dev)
            st["epoch"] = st.get("epoch", 0) + 1
        self.sync_lr()
        # st["segs"] = (begin, end, group index, beta1, beta2, eps, weight_decay, mode): the _ex record; today's entry points, which
        # run while no group is decoupled, take it without the mode
        clip4 = None
        if self._clipping():
            self._check_max_grad_norm(self.max_grad_norm)
            clip4, ws = self._clip_buffers(st, arena_p.device, len(st["segs"]))
            ops.grad_norm_segments(arena_g, st["segs"], self.max_grad_norm, self.skip_nonfinite, clip4, ws)
        if self._any_decoupled():
            ops.adam_step_segments_dev_ex(arena_p, arena_g, st["exp_avg"], st["exp_avg_sq"], st["segs"], st["lr_dev"], st["state3"], clip4)
        elif clip4 is None:
            ops.adam_step_segments_dev(arena_p, arena_g, st["exp_avg"], st["exp_avg_sq"], st["segs_coupled"], st["lr_dev"], st["state3"])
        else:
            ops.adam_step_segments_dev_clip(arena_p, arena_g, st["exp_avg"], st["exp_avg_sq"], st["segs_coupled"], st["lr_dev"],
                                            st["state3"], clip4)

    # ---- max_grad_norm / skip_nonfinite: the device record and the norm's workspace
    def _clip_buffers(self, st, device, n_segments: int):
        """(clip4, workspace) of one model's state: created in an eager step, never inside a capture (a captured step holds their
        addresses).  clip4 is zeroed once - its skipped_total counts from then on."""
        if "clip4" not in st or st.get("clip_segments", 0) < n_segments:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("Adam: max_grad_norm / skip_nonfinite need one eager step before capturing (the clip record and the "
                                   "norm's workspace are created there, never inside a capture)")
            st.setdefault("clip4", torch.zeros(4, dtype=torch.float32, device=device))
            with torch.cuda.device(device):
                st["clip_ws"] = torch.empty(ops.grad_norm_workspace_bytes(n_segments), dtype=torch.uint8, device=device)
            st["clip_segments"] = n_segments
        return st["clip4"], st["clip_ws"]

    def clip_record(self, model) -> torch.Tensor:
        """The device record {norm, coef, skipped, skipped_total} of ``model``'s last step (four floats; no synchronisation)."""
        st = self._flat.get(id(model))
        if st is None or "clip4" not in st:
            raise RuntimeError("Adam.clip_record: no step with max_grad_norm or skip_nonfinite has run for this model yet")
        return st["clip4"]

    def grad_clip_report(self) -> List[dict]:
        """One {"norm", "coef", "skipped", "skipped_total"} per model, read back from the device (this synchronises)."""
        out = []
        for model in self._owners():
            st = self._flat.get(id(model))
            if st is not None and "clip4" in st:
                norm, coef, skipped, total = st["clip4"].cpu().tolist()
                out.append({"norm": norm, "coef": coef, "skipped": bool(skipped), "skipped_total": int(total)})
        return out

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group_of = {id(p): g for g in self.param_groups for p in g["params"]}
        for model in self._owners():
            model.ensure_layout()
            arena_g, entries = model.grad_arena()
            # a parameter takes part when it is in a group and holds a gradient; torch skips every other one, and so do we
            groups = [group_of.get(id(p)) for (p, _, _) in entries]
            have = [g is not None and p.grad is not None for (p, _, _), g in zip(entries, groups)]
            if not any(have):
                continue                              # nothing was back-propagated: torch skips too
            for (p, off, n), h in zip(entries, have):
                if h and p.grad.data_ptr() != arena_g.data_ptr() + 4 * off:
                    raise RuntimeError("every trainable parameter must hold the gradient written by the "
                                       "module's backward (a view of its gradient arena)")
            arena_p = model.param_arena()
            if self.capturable == "segments" and id(model) not in self._flat and torch.cuda.is_current_stream_capturing():
                # (before the moments exist: their zero fill would be captured, not run)
                raise RuntimeError("Adam(capturable='segments'): run one eager step before capturing (the moments and the device "
                                   "state are created there, never inside a capture)")
            st = self._state_for(model, arena_p, len(entries))
            steps = [s + 1 if h else s for s, h in zip(st["steps"], have)]
            # the reference-shaped step: one group, every arena parameter in it with a gradient, one step count
            whole = len(self.param_groups) == 1 and all(have) and len(set(steps)) == 1
            if self.capturable == "segments":
                # (the counts stay the ones the device table was built from: the table itself is advanced by the launch)
                st.setdefault("lr_host", [])
                self._step_segments_dev(st, entries, have, arena_p, arena_g)
                for (p, _, _), h in zip(entries, have):
                    if h:
                        torch.autograd.graph.increment_version(p)
                continue
            if self.capturable and not whole:
                raise NotImplementedError("Adam(capturable=True) cannot skip parameters (refused at step()): a parameter without a "
                                          "gradient, or with a step count of its own, needs the segmented step, which takes its "
                                          "segments from the host; use capturable=False for frozen or later-unfrozen parameters")
            if self._clipping():
                # the segmented forms over the plan's segments, whatever the plan (a segment equals mvg_adam_step over its slice
                # bit for bit): the norm over exactly those segments, then the update that reads its record
                if self.capturable:
                    raise ValueError("Adam(capturable=True) takes neither max_grad_norm nor skip_nonfinite (set after construction): "
                                     "use capturable='segments'")
                self._check_max_grad_norm(self.max_grad_norm)
                segs = plan_segments([(off, n) for (_, off, n) in entries], [self._hyper(g) if g is not None else None for g in groups],
                                     have, steps)
                clip4, ws = self._clip_buffers(st, arena_p.device, len(segs))
                ops.grad_norm_segments(arena_g, [(s.begin, s.end) for s in segs], self.max_grad_norm, self.skip_nonfinite, clip4, ws)
                if self.skip_nonfinite and float(clip4[2].item()) != 0.0:      # (the one synchronisation of this mode)
                    continue                                                    # skipped: no update, the step counts stay
                st["steps"] = steps
                st["step"] = max(steps)
                self._step_segments_host(arena_p, arena_g, st, segs, clip4)
                for (p, _, _), h in zip(entries, have):
                    if h:
                        torch.autograd.graph.increment_version(p)
                continue
            st["steps"] = steps
            st["step"] = max(steps)
            if self.capturable:
                g = self.param_groups[0]
                if "lr_dev" not in st:
                    if torch.cuda.is_current_stream_capturing():
                        raise RuntimeError("Adam(capturable=True): run one eager step before capturing (its device state is created then)")
                    st["lr_dev"] = torch.full((1,), float(g["lr"]), dtype=torch.float32, device=arena_p.device)
                    st["lr_host"] = float(g["lr"])
                    # {step, 1 - beta1^step, sqrt(1 - beta2^step)}: advanced on the device by every (captured or eager) step
                    st["state3"] = torch.tensor([float(st["step"] - 1), 0.0, 0.0], dtype=torch.float32).to(arena_p.device)
                self.sync_lr()
                step_dev = ops.adamw_step_dev if g["decoupled_weight_decay"] else ops.adam_step_dev
                step_dev(arena_p, arena_g, st["exp_avg"], st["exp_avg_sq"], st["lr_dev"], st["state3"], float(g["betas"][0]),
                         float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]))
            elif whole:
                g = self.param_groups[0]
                step_host = ops.adamw_step if g["decoupled_weight_decay"] else ops.adam_step
                step_host(arena_p, arena_g, st["exp_avg"], st["exp_avg_sq"], float(g["lr"]), float(g["betas"][0]),
                          float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]), st["step"])
            else:
                segs = plan_segments([(off, n) for (_, off, n) in entries], [self._hyper(g) if g is not None else None for g in groups],
                                     have, steps)
                self._step_segments_host(arena_p, arena_g, st, segs, None)
            # the parameters alias the arena through `.data` (their own version counters): mark them modified, as an
            # in-place torch op would (the inference path's cache of split weights keys on the version)
            for (p, _, _), h in zip(entries, have):
                if h:
                    torch.autograd.graph.increment_version(p)
        return loss

    # The moments live in flat buffers that mirror the model's parameter arena (one launch updates all of
    # them), not in ``self.state``; checkpoints carry them under one extra key so that a resumed run keeps
    # its bias correction and moments (the reference itself checkpoints the model only, trainer.py:91-96).
    # "steps" holds one count per arena parameter, in arena order; "step" (their maximum) is what entries held before
    # per-parameter counts, and an entry with "step" alone still loads: every parameter gets that count.
    def state_dict(self):
        sd = super().state_dict()
        flat = []
        for model in self._owners():
            st = self._flat.get(id(model))
            if st is not None:
                if "seg_of" in st:                  # capturable="segments": one device counter per segment
                    self._pull_steps(st)
                elif "state3" in st:                # capturable: the device counter is the truth (graph replays advance it)
                    st["step"] = int(round(float(st["state3"][0].item())))
                    st["steps"] = [st["step"]] * len(st["steps"])
                flat.append({"step": st["step"], "steps": list(st["steps"]), "exp_avg": st["exp_avg"].detach().clone(),
                             "exp_avg_sq": st["exp_avg_sq"].detach().clone()})
        sd["mvg_arena_state"] = flat
        return sd

    def load_state_dict(self, state_dict):
        sd = dict(state_dict)
        flat = sd.pop("mvg_arena_state", None)
        super().load_state_dict(sd)
        for g in self.param_groups:                 # (a checkpoint written before the flag existed: the coupled decay it ran)
            g.setdefault("decoupled_weight_decay", False)
        self._flat.clear()
        self._pending = [dict(e) for e in flat] if flat else None


class AdamW(Adam):
    """``Adam`` with torch.optim.AdamW's defaults: ``weight_decay=1e-2`` and ``decoupled_weight_decay=True``.  Everything else -
    parameter groups (a group may set ``decoupled_weight_decay=False`` or ``weight_decay=0``), frozen parameters, ``capturable``,
    ``max_grad_norm``, ``skip_nonfinite``, the checkpoint format - is Adam's."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, capturable=False, max_grad_norm=None,
                 skip_nonfinite=False, decoupled_weight_decay=True):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, capturable=capturable,
                         max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite, decoupled_weight_decay=decoupled_weight_decay)
