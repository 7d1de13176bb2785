"""Shared cases of the fused optimizer tests (tests/test_optim_cpu.py, tests/test_gpu_optim.py): the tensor sizes that
make the chunk and table logic of csrc/optim_pack.h go wrong if it can, the hyper-parameter cases, seeded values, and the
reference: torch.optim.Adam / AdamW(foreach=False) on the CPU, in fp64 (the truth) and in fp32 (whose distance from the
truth, e_ref, sets the error bars).  reference() results are cached: computed once per (case, clip) and never modified."""
import functools

import torch

from aaclip_hip import _lib

CHUNK, TABLE_TENSORS, TABLE_BLOCKS = _lib.OPTIM_CHUNK, _lib.OPTIM_TABLE_TENSORS, _lib.OPTIM_TABLE_BLOCKS

# index of the parameter whose grad stays None, of the zero-element one and of the one stepped from misaligned views
EDGE_SIZES = [1, 3, 4, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5]
GRADLESS, EMPTY, MISALIGNED = len(EDGE_SIZES), len(EDGE_SIZES) + 1, len(EDGE_SIZES) + 2
SIZES = EDGE_SIZES + [37, 0, 1027] + [1 + i % 7 for i in range(3 * TABLE_TENSORS + 1)]

# name -> (torch class name, [(first tensor, lr, weight_decay)] groups, betas)
HYPER = {
    "stage1": ("Adam", [(0, 1e-5, 0.0)], (0.5, 0.999)),
    "stage2": ("AdamW", [(0, 5e-4, 1e-4), (len(SIZES) // 2, 5e-5, 1e-3)], (0.9, 0.999)),
    "large_lr": ("AdamW", [(0, 0.1, 1e-2)], (0.9, 0.999)),
    "coupled": ("Adam", [(0, 1e-3, 1e-2)], (0.9, 0.999)),
}
STEPS = 3
LOADED_STEP = 1000            # the "loaded" variant: one step from a state with step = 1000 and seeded moments


def values(seed, scale=1.0, sizes=SIZES):
    """seeded fp32 tensors of the case's sizes (CPU)"""
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=gen, dtype=torch.float32) * scale for n in sizes]


def initial(loaded):
    """-> (p, m, v, step): fp32 CPU lists; zero moments and step 0, or seeded moments and LOADED_STEP"""
    p = values(1, 0.05)
    if not loaded:
        return p, [torch.zeros_like(t) for t in p], [torch.zeros_like(t) for t in p], 0
    return p, values(2, 0.01), [t.abs() * 1e-3 for t in values(3)], LOADED_STEP


def gradients(step, scale=0.02):
    """the fp32 gradients of step `step` (0-based); the GRADLESS entry is None"""
    g = values(100 + step, scale)
    g[GRADLESS] = None
    return g


def param_groups(params, case):
    _, groups, _ = HYPER[case]
    starts = [first for first, _, _ in groups] + [len(params)]
    return [{"params": params[starts[i]:starts[i + 1]], "lr": lr, "weight_decay": wd}
            for i, (_, lr, wd) in enumerate(groups)]


def build(cls, params, case, **extra):
    return cls(param_groups(params, case), betas=HYPER[case][2], **extra)


def torch_class(case):
    return getattr(torch.optim, HYPER[case][0])


def fused_class(case):
    from aaclip_hip import optim
    return {"Adam": optim.FusedAdam, "AdamW": optim.FusedAdamW}[HYPER[case][0]]


def state_dict_of(optimizer, m, v, step):
    """a state dict in torch's layout that puts (m, v, step) under every parameter (including the GRADLESS one)"""
    sd = optimizer.state_dict()
    sd["state"] = {i: {"step": torch.tensor(float(step), dtype=torch.float32), "exp_avg": m[i].clone(),
                       "exp_avg_sq": v[i].clone()} for i in range(len(m))}
    return sd


def clip_coef(norm, max_norm):
    """torch.nn.utils.clip_grad_norm_'s coefficient"""
    return min(1.0, max_norm / (norm + 1e-6))


def run_torch(case, dtype, loaded=False, grad_scale=0.02, max_norm=None, poison=None):
    """torch's optimizer on the CPU in `dtype`, started from the fp32 values: -> {"p", "m", "v": lists after the last
    step, "norms": clip_grad_norm_'s returned norm per step}.  max_norm: clip_grad_norm_ before every step.
    poison: (tensor index, element) of the first step's gradient that is set to inf."""
    p0, m0, v0, step0 = initial(loaded)
    params = [torch.nn.Parameter(t.to(dtype)) for t in p0]
    opt = build(torch_class(case), params, case, foreach=False)
    if loaded:
        opt.load_state_dict(state_dict_of(opt, [t.to(dtype) for t in m0], [t.to(dtype) for t in v0], step0))
    norms = []
    for s in range(1 if loaded else STEPS):
        for p, g in zip(params, gradients(s, grad_scale)):
            p.grad = None if g is None else g.to(dtype)
        if poison is not None and s == 0:
            params[poison[0]].grad[poison[1]] = float("inf")
        if max_norm is not None:
            norms.append(torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False).detach().clone())
        opt.step()
    zeros = [torch.zeros_like(p) for p in params]
    return {"p": [p.detach() for p in params],
            "m": [opt.state[p].get("exp_avg", z) for p, z in zip(params, zeros)],
            "v": [opt.state[p].get("exp_avg_sq", z) for p, z in zip(params, zeros)],
            "norms": norms}


@functools.lru_cache(maxsize=None)
def reference(case, loaded=False, grad_scale=0.02, max_norm=None, poison=None):
    """-> (truth, e_ref, bars): truth = run_torch in fp64; e_ref[k], k in p / m / v / norm = the largest absolute
    difference of the same torch optimizer in fp32 from the truth over the whole case; bars[k] = max(4 e_ref, 4 * 2^-24 *
    max |truth|): four roundings' worth of reordering, and four half-ulps of the largest element where torch happens to be
    exact.  Non-finite entries (poison) are left out of the maxima."""
    truth = run_torch(case, torch.float64, loaded, grad_scale, max_norm, poison)
    ref32 = run_torch(case, torch.float32, loaded, grad_scale, max_norm, poison)
    e_ref, bars = {}, {}
    for k in ("p", "m", "v", "norms"):
        err = top = 0.0
        for t, r in zip(truth[k], ref32[k]):
            t, r = t.reshape(-1), r.reshape(-1).double()
            ok = torch.isfinite(t) & torch.isfinite(r)
            if ok.any():
                err = max(err, float((t[ok] - r[ok]).abs().max()))
                top = max(top, float(t[ok].abs().max()))
        e_ref[k] = err
        bars[k] = max(4 * err, 4 * 2.0 ** -24 * top)
    return truth, e_ref, bars


def errors(got, truth):
    """largest absolute difference per list entry pair, over the finite entries of the truth; got: fp32 lists"""
    worst = 0.0
    for a, t in zip(got, truth):
        a, t = a.detach().cpu().reshape(-1).double(), t.reshape(-1)
        ok = torch.isfinite(t)
        if ok.any():
            worst = max(worst, float((a[ok] - t[ok]).abs().max()))
    return worst


# ------------------------------------------------------------------- fp64 torch stand-ins for the two engine calls
def standin_grad_norm(grads, max_norm, record=None, workspace=None):
    from aaclip_hip import engine
    if isinstance(grads, engine.OptimPack):
        grads = grads.grads
    total = torch.sqrt(sum((g.double() ** 2).sum() for g in grads)) if grads else torch.zeros((), dtype=torch.float64)
    norm = total.float()
    coef = (max_norm / (norm + 1e-6)).clamp(max=1.0)
    if record is None:
        record = torch.empty(2, dtype=torch.float32)
    record[0], record[1] = norm, coef
    return record


def standin_adam_step(params, grads=None, exp_avgs=None, exp_avg_sqs=None, group_of=None, groups=(), record=None):
    """include/aaclip.h aaclip_optim_adam_step in fp64, stored back into the tensors' own dtype"""
    from aaclip_hip import engine
    if isinstance(params, engine.OptimPack):
        params, grads, exp_avgs, exp_avg_sqs, group_of = (params.params, params.grads, params.exp_avgs,
                                                          params.exp_avg_sqs, params.group_of)
    assert 1 <= len(groups) <= _lib.OPTIM_MAX_GROUPS
    coef = 1.0 if record is None else record[1].double()
    for p, g, m, v, k in zip(params, grads, exp_avgs, exp_avg_sqs, group_of):
        h = groups[k]
        g64, p64, m64, v64 = g.double() * coef, p.double(), m.double(), v.double()
        if h["decoupled"]:
            p64 = p64 * (1 - h["lr"] * h["weight_decay"])
        else:
            g64 = g64 + h["weight_decay"] * p64
        m64 = h["beta1"] * m64 + (1 - h["beta1"]) * g64
        v64 = h["beta2"] * v64 + (1 - h["beta2"]) * g64 * g64
        bc1, bc2 = 1 - h["beta1"] ** h["step"], 1 - h["beta2"] ** h["step"]
        p64 = p64 - (h["lr"] / bc1) * m64 / (v64.sqrt() / bc2 ** 0.5 + h["eps"])
        p.copy_(p64), m.copy_(m64), v.copy_(v64)


def install_standins(monkeypatch, counts=None):
    """Put the stand-ins on aaclip_hip.engine (and let CPU tensors pass its device check); counts (a dict):
    counts[name] += 1 per call."""
    from aaclip_hip import engine

    def counted(name, fn):
        def call(*args, **kwargs):
            counts[name] = counts.get(name, 0) + 1
            return fn(*args, **kwargs)
        return fn if counts is None else call

    monkeypatch.setattr(engine, "require_gpu", lambda t, what: None)
    monkeypatch.setattr(engine, "optim_grad_norm", counted("optim_grad_norm", standin_grad_norm))
    monkeypatch.setattr(engine, "optim_adam_step", counted("optim_adam_step", standin_adam_step))
