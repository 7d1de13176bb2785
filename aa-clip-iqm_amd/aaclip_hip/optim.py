"""FusedAdam / FusedAdamW: torch.optim.Adam / AdamW whose step() is the library's multi-tensor kernels (csrc/optim.hip).

One step reads p, g, m, v of every parameter once and writes p, m, v once, in as few launches as the tensor list needs
(engine.optim_adam_step), instead of torch's dozen `foreach` passes.  With max_grad_norm the step is clipped the way
torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm) followed by step() would be: the 2-norm over every parameter
of every group that has a gradient (engine.optim_grad_norm), clip_coef = min(1, max_norm / (norm + 1e-6)).  The
coefficient stays on the device, so nothing synchronises; `optimizer.grad_norm` is the norm of the last step as a device
tensor.  One difference from clip_grad_norm_: the gradients in memory are NOT rescaled, the coefficient is applied as
they are read.

state_dict() / load_state_dict() use torch's layout (state[i] = {"step": fp32 scalar tensor, "exp_avg", "exp_avg_sq"},
param_groups with torch's keys), so a checkpoint written with torch.optim.Adam / AdamW resumes here and the other way
round.  param_groups[i]["lr"] is read at every step: torch's schedulers work unchanged.

Parameters, gradients and state are fp32, contiguous and on the GPU; anything else raises before any launch.  There is
no fallback to torch's step.  amsgrad, maximize, capturable and differentiable are not implemented.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import engine

_UNSUPPORTED = ("amsgrad", "maximize", "capturable", "differentiable")


class _FusedAdamBase(torch.optim.Optimizer):
    _torch_class = None       # whose defaults, hyper-parameter checks and state layout this class takes over
    _decoupled = False
    max_grad_norm = None
    _record = None            # fp32 [2] on the device: total_norm, clip_coef
    _workspace = None
    _plan = None              # the packed tensor list of the last step (_build_plan)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=None, amsgrad=False, *,
                 maximize=False, capturable=False, differentiable=False, max_grad_norm: Optional[float] = None):
        flags = dict(amsgrad=amsgrad, maximize=maximize, capturable=capturable, differentiable=differentiable)
        for name in _UNSUPPORTED:
            if flags[name]:
                raise NotImplementedError(f"{type(self).__name__}: {name}=True is not implemented")
        if torch.is_tensor(lr):
            raise NotImplementedError(f"{type(self).__name__}: a tensor lr is not implemented (it needs capturable)")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm} (None or a number above 0)")
        kwargs = dict(lr=lr, betas=betas, eps=eps)
        if weight_decay is not None:
            kwargs["weight_decay"] = weight_decay
        # torch's own constructor checks the hyper-parameters and supplies its defaults, so that param_groups carries
        # exactly the keys torch's optimizer of this version writes into a checkpoint
        defaults = dict(self._torch_class([torch.nn.Parameter(torch.zeros(1))], **kwargs).defaults)
        super().__init__(params, defaults)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)

    @property
    def grad_norm(self) -> Optional[torch.Tensor]:
        """0-dim fp32 device tensor: the gradient norm the last clipped step() measured (before clipping); None before
        the first such step.  Reading its value synchronises; step() never does."""
        return None if self._record is None else self._record[0]

    def load_state_dict(self, state_dict) -> None:
        """torch's; the step counts are then kept on the host, where step() reads them without a synchronisation (a
        checkpoint loaded with map_location=<gpu> carries them as device tensors)."""
        super().load_state_dict(state_dict)
        self._plan = None
        self._check_groups()
        for state in self.state.values():
            if "step" in state:
                step = state["step"]
                state["step"] = (step.detach().to("cpu", torch.float32) if torch.is_tensor(step)
                                 else torch.tensor(float(step), dtype=torch.float32))

    def _check_groups(self):
        for gi, group in enumerate(self.param_groups):
            for name in _UNSUPPORTED:
                if group.get(name, False):
                    raise NotImplementedError(f"{type(self).__name__}: param_groups[{gi}] sets {name}=True")

    def _build_plan(self):
        """Check every parameter that has a gradient (every refusal happens here, before any state changes and before
        any launch), create missing state, and pack the tensor list once; step() reuses the plan while the same
        parameters step from the same addresses.  None when nothing has a gradient."""
        name = type(self).__name__
        found = []                     # (group index, parameter, it steps)
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                steps = p.grad is not None
                if steps:
                    engine._optim_tensor(p, name)
                    engine._optim_tensor(p.grad, name + " (gradient)", like=p)
                    state = self.state.get(p, {})
                    for key in ("exp_avg", "exp_avg_sq"):
                        if key in state:
                            engine._optim_tensor(state[key], f"{name} ({key})", like=p)
                found.append((gi, p, steps and p.numel() != 0))
        work = [(gi, p) for gi, p, steps in found if steps]
        if not work:
            return None
        if any(p.device != work[0][1].device for _, p in work):
            raise ValueError(f"{name}: the parameters must be on one device")
        counts, buckets, group_of = [], {}, []
        for gi, p in work:
            state = self.state[p]
            if len(state) == 0:
                state["step"] = torch.tensor(0.0, dtype=torch.float32)
                state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            counts.append(float(state["step"]))
            group_of.append(buckets.setdefault((gi, int(counts[-1])), len(buckets)))
        plan = _Plan()
        # one host tensor holds every step count; state[p]["step"] is a 0-dim view of it, so one add advances them all
        plan.steps = torch.tensor(counts, dtype=torch.float32)
        for j, (_, p) in enumerate(work):
            self.state[p]["step"] = plan.steps[j]
        plan.buckets = [[gi, step] for (gi, step), _ in sorted(buckets.items(), key=lambda kv: kv[1])]
        lists = ([p for _, p in work], [p.grad for _, p in work], [self.state[p]["exp_avg"] for _, p in work],
                 [self.state[p]["exp_avg_sq"] for _, p in work])
        plan.all = engine.OptimPack(*lists, group_of, name)
        # one call per engine.OPTIM_MAX_GROUPS hyper-parameter sets: one call unless parameters of a group have taken
        # different numbers of steps (a parameter whose grad was None for a while)
        G = engine.OPTIM_MAX_GROUPS
        where = [(plan.all, j) for j in range(len(work))]
        plan.parts = [(plan.all, 0)]
        if len(plan.buckets) > G:
            plan.parts = []
            for first in range(0, len(plan.buckets), G):
                pick = [j for j, k in enumerate(group_of) if first <= k < first + G]
                part = engine.OptimPack(*[[lst[j] for j in pick] for lst in lists], [group_of[j] - first for j in pick], name)
                plan.parts.append((part, first))
                for i, j in enumerate(pick):
                    where[j] = (part, i)
        plan.rows, j = [], 0
        for gi, p, steps in found:
            if steps:
                state = self.state[p]
                plan.rows.append((p, p.data_ptr(), j, where[j], state, state["exp_avg"], state["exp_avg_sq"], state["step"]))
                j += 1
            else:
                plan.rows.append((p, 0, -1, None, None, None, None, None))
        return plan

    def _plan_holds(self, plan) -> bool:
        """the same parameters step from the same addresses with the same state tensors; gradients that are new
        tensors are checked and put into the packed list"""
        k, rows, grads = 0, plan.rows, plan.all.grads
        for group in self.param_groups:
            for p in group["params"]:
                if k == len(rows):
                    return False
                q, ptr, j, where, state, m, v, count = rows[k]
                k += 1
                g = p.grad
                if q is not p:
                    return False
                if j < 0:
                    if g is not None and p.numel() != 0:
                        return False
                    continue
                if (g is None or p.data_ptr() != ptr or state.get("exp_avg") is not m or state.get("exp_avg_sq") is not v
                        or state.get("step") is not count):
                    return False
                if g is not grads[j]:
                    # torch keeps a gradient's dtype, device and shape equal to its parameter's; the layout is free
                    if g.layout is not torch.strided or not g.is_contiguous():
                        engine._optim_tensor(g, type(self).__name__ + " (gradient)", like=p)
                    plan.all.set_grad(j, g)
                    if where[0] is not plan.all:
                        where[0].set_grad(where[1], g)
        return k == len(rows)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_groups()
        plan = self._plan
        if plan is None or not self._plan_holds(plan):
            plan = self._plan = self._build_plan()
        if plan is None:
            return loss
        plan.steps += 1
        hyper = []
        for bucket in plan.buckets:
            bucket[1] += 1
            group = self.param_groups[bucket[0]]
            hyper.append({"lr": float(group["lr"]), "beta1": group["betas"][0], "beta2": group["betas"][1],
                          "eps": group["eps"], "weight_decay": group["weight_decay"], "step": bucket[1],
                          # torch versions whose AdamW is Adam(decoupled_weight_decay=True) carry the key in the group
                          "decoupled": bool(group.get("decoupled_weight_decay", self._decoupled))})
        record = None
        if self.max_grad_norm is not None:
            dev, need = plan.all.device, plan.all.norm_workspace_bytes
            if self._record is None or self._record.device != dev:
                self._record = torch.zeros(engine.OPTIM_RECORD_FLOATS, dtype=torch.float32, device=dev)
            if self._workspace is None or self._workspace.device != dev or self._workspace.numel() < need:
                self._workspace = torch.empty(need, dtype=torch.uint8, device=dev)
            record = engine.optim_grad_norm(plan.all, self.max_grad_norm, self._record, self._workspace)
        G = engine.OPTIM_MAX_GROUPS
        for pack, first in plan.parts:
            engine.optim_adam_step(pack, groups=hyper[first:first + G], record=record)
        return loss


class _Plan:
    """what step() keeps from one call to the next: steps (fp32 host tensor, one count per stepping parameter), buckets
    ([param group, step] per hyper-parameter set), all (engine.OptimPack of every stepping parameter), parts ([(pack,
    first bucket)] per optim_adam_step call) and rows (one per parameter of every group, in order)"""
    __slots__ = ("steps", "buckets", "all", "parts", "rows")


class FusedAdam(_FusedAdamBase):
    """torch.optim.Adam(params, lr, betas, eps, weight_decay=0) on the fused kernels; the weight decay joins the gradient
    (g + weight_decay * p, after clipping).  max_grad_norm: clip inside step(), see the module docstring."""
    _torch_class = torch.optim.Adam
    _decoupled = False


class FusedAdamW(_FusedAdamBase):
    """torch.optim.AdamW(params, lr, betas, eps, weight_decay=1e-2) on the fused kernels; the weight decay is decoupled
    (p * (1 - lr * weight_decay)).  max_grad_norm: clip inside step(), see the module docstring."""
    _torch_class = torch.optim.AdamW
    _decoupled = True
