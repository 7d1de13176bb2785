"""Seeded cases and the fp64 reference shared by tests/test_cross_rows_backward_cpu.py and
tests/test_gpu_cross_rows_backward.py (aaclip_cross_rows_backward, autograd.cross_rows, autograd.iqm_visual_rows).

The reference is the forward formula of aaclip_cross_rows, s = qt x^T, p = softmax_j s, out = p x, differentiated by
torch autograd in fp64."""
import functools

import torch
import torch.nn.functional as F

from aaclip_hip import synth

NONE, LEAKY, RELU = 0, 1, 2              # AACLIP_ACT_*
F32, F16 = 0, 1                          # AACLIP_F32, AACLIP_F16
MAX_SLICES = 128                         # csrc/kernels.h CRB_MAX_SLICES (engine.CROSS_ROWS_BACKWARD_MAX_SLICES)

# name -> dict(B, R, Lk, Dk) plus what departs from: fp32 rows, no activation, overwrite, both outputs, unit scores.
# `peak`: every qt row is rescaled so that its largest score is `peak` (the smallest is then near -peak).
CASES = {
    "one_key": dict(B=1, R=4, Lk=1, Dk=256),                                   # p = 1, ds = 0, d_qt = 0 exactly
    "below_one_tile": dict(B=2, R=16, Lk=63, Dk=256),
    "ragged_tiles": dict(B=3, R=8, Lk=197, Dk=512),
    "tail_slice_of_one_row": dict(B=2, R=12, Lk=64 * MAX_SLICES + 1, Dk=768),  # slices of 128 keys, the last holds 1
    "widest_rows": dict(B=2, R=16, Lk=300, Dk=1024),
    "production": dict(B=2, R=16, Lk=5476, Dk=768),
    "nearly_one_hot": dict(B=2, R=8, Lk=197, Dk=512, peak=80.0),
    "fp16_rows": dict(B=2, R=16, Lk=150, Dk=768, code=F16),
    "leaky": dict(B=2, R=16, Lk=150, Dk=256, act=LEAKY),
    "relu": dict(B=2, R=8, Lk=100, Dk=512, act=RELU),
    "accumulate": dict(B=2, R=16, Lk=150, Dk=256, accumulate=True),
    "d_qt_only": dict(B=2, R=4, Lk=150, Dk=256, outs="d_qt"),
    "d_x_only": dict(B=2, R=4, Lk=150, Dk=256, outs="d_x"),
}


def rnd(name, shape, std=1.0):
    return synth.randn("crb." + name, shape, std, 31)


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.isfinite(a).all()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def slope_mask(x, act):
    """the activation's derivative from the sign of its OUTPUT x: 1 for x > 0; 0.01 (LEAKY) / 0 (RELU) for x <= 0"""
    neg = {NONE: 1.0, LEAKY: 0.01, RELU: 0.0}[act]
    return torch.where(x > 0, torch.ones((), dtype=x.dtype), torch.full((), neg, dtype=x.dtype))


def case_inputs(name):
    """-> dict: qt, d_out [B*R, Dk] fp32, x [B*Lk, Dk] in the case's dtype, base [B*Lk, Dk] fp32 (accumulate cases)"""
    c = CASES[name]
    B, R, Lk, Dk = c["B"], c["R"], c["Lk"], c["Dk"]
    x = rnd(name + ".x", (B * Lk, Dk))
    if c.get("act", NONE) != NONE:            # negative values and exact zeros in every row
        x[:, ::7] = 0.0
        if c["act"] == LEAKY:
            x = torch.where(x > 0, x, 0.01 * x)
    if c.get("code", F32) == F16:
        x = x.half()
    qt = rnd(name + ".qt", (B * R, Dk), 1.5 * Dk ** -0.5)
    if c.get("peak") is not None:
        s = qt.double().view(B, R, Dk) @ x.double().view(B, Lk, Dk).transpose(1, 2)
        qt = (qt.double().view(B, R, Dk) * (c["peak"] / s.amax(dim=-1, keepdim=True))).view(B * R, Dk).float()
    t = {"qt": qt, "x": x, "d_out": rnd(name + ".d_out", (B * R, Dk))}
    if c.get("accumulate"):
        t["base"] = rnd(name + ".base", (B * Lk, Dk), 0.05)
    return t


def autograd_reference(qt, x, d_out, B, R, Lk, Dk, dtype=torch.float64):
    """-> (d_qt [B*R, Dk], d_x [B*Lk, Dk], out [B*R, Dk]) of the forward formula in `dtype` on the CPU"""
    q = qt.to(dtype).view(B, R, Dk).requires_grad_(True)
    xx = x.to(dtype).view(B, Lk, Dk).requires_grad_(True)
    out = torch.softmax(q @ xx.transpose(1, 2), dim=-1) @ xx
    out.backward(d_out.to(dtype).view(B, R, Dk))
    return q.grad.reshape(B * R, Dk), xx.grad.reshape(B * Lk, Dk), out.detach().reshape(B * R, Dk)


def want_of(name, d_qt, d_x, t):
    """what the entry point is to return for the case, from the plain gradients: the slope mask and the base applied"""
    c = CASES[name]
    d_x = d_x * slope_mask(t["x"].to(d_x.dtype), c.get("act", NONE))
    if c.get("accumulate"):
        d_x = t["base"].to(d_x.dtype) + d_x
    outs = c.get("outs", "both")
    return {"d_qt": d_qt if outs != "d_x" else None, "d_x": d_x if outs != "d_qt" else None}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (inputs, fp64 expectations {d_qt, d_x}): computed once, shared, never modified"""
    c = CASES[name]
    t = case_inputs(name)
    d_qt, d_x, _ = autograd_reference(t["qt"], t["x"], t["d_out"], c["B"], c["R"], c["Lk"], c["Dk"])
    return t, want_of(name, d_qt, d_x, t)


def step_sequence(qt, x, d_out, B, R, Lk, Dk):
    """The passes of csrc/iqm_backward.hip in fp64 torch -> (d_qt, d_x)"""
    q, xx, do = (v.double().view(B, -1, Dk) for v in (qt, x, d_out))
    S, G = xx @ q.transpose(1, 2), xx @ do.transpose(1, 2)            # pass A: [B, Lk, R] each
    m = S.amax(dim=1, keepdim=True)                                   # statistics
    e = torch.exp(S - m)
    linv = 1.0 / e.sum(dim=1, keepdim=True)
    delta = (e * linv * G).sum(dim=1, keepdim=True)
    P = e * linv                                                      # pass B
    dS = P * (G - delta)
    d_x = torch.cat([P, dS], dim=2) @ torch.cat([do, q], dim=1)
    d_qt = dS.transpose(1, 2) @ xx
    return d_qt.reshape(B * R, Dk), d_x.reshape(B * Lk, Dk)


# ---------------------------------------------------------------------------------------------- the folding check
FOLD = dict(B=2, nq=2, H=8, Lk=150, h=256)


def fold_inputs():
    B, nq, H, Lk, h = (FOLD[k] for k in ("B", "nq", "H", "Lk", "h"))
    return {"x": rnd("fold.x", (B, Lk, h)), "q": rnd("fold.q", (B, nq, h)),
            "Wk": rnd("fold.Wk", (h, h), h ** -0.5), "bk": rnd("fold.bk", (h,), 0.1),
            "Wv": rnd("fold.Wv", (h, h), h ** -0.5), "bv": rnd("fold.bv", (h,), 0.1),
            "P": rnd("fold.P", (h, h), h ** -0.5), "pb": rnd("fold.pb", (h,), 0.1),
            "d_ctx": rnd("fold.d_ctx", (B, nq, h))}


def fold_reference():
    """The reference's cross-attention in fp64 (visual_feature_proj, key / value Linear, per-head softmax) ->
    (ctx, d x, d W_k, d b_k)"""
    B, nq, H, Lk, h = (FOLD[k] for k in ("B", "nq", "H", "Lk", "h"))
    t = {k: v.double() for k, v in fold_inputs().items()}
    for k in ("x", "Wk", "bk"):
        t[k].requires_grad_(True)
    e = t["x"] @ t["P"].t() + t["pb"]
    K = (e @ t["Wk"].t() + t["bk"]).view(B, Lk, H, h // H).transpose(1, 2)
    V = (e @ t["Wv"].t() + t["bv"]).view(B, Lk, H, h // H).transpose(1, 2)
    Q = t["q"].view(B, nq, H, h // H).transpose(1, 2)
    p = torch.softmax(Q @ K.transpose(-1, -2) / (h // H) ** 0.5, dim=-1)
    ctx = (p @ V).transpose(1, 2).reshape(B, nq, h)
    ctx.backward(t["d_ctx"])
    return ctx.detach(), t["x"].grad, t["Wk"].grad, t["bk"].grad


# ---------------------------------------------------------------------------------------------- iqm_visual_rows
def visual_rows_oracle(taps, weights, ln_w, ln_b, relu, d_rows, dtype):
    """query_adapters[k](ln_post(tap k)) without the CLS row, concatenated (reference model/adapter.py:205-211), in
    `dtype` on the CPU, contracted with d_rows -> (rows, [d tap], [d weight], smallest |pre-activation|)"""
    ts = [t.detach().cpu().to(dtype).requires_grad_(True) for t in taps]
    ws = [w.detach().cpu().to(dtype).requires_grad_(True) for w in weights]
    rows, zmin = [], float("inf")
    for t, w in zip(ts, ws):
        z = F.layer_norm(t, (t.shape[-1],), ln_w.detach().cpu().to(dtype), ln_b.detach().cpu().to(dtype), 1e-5) @ w.t()
        zmin = min(zmin, float(z[:, 1:].detach().abs().min()))
        rows.append((F.leaky_relu(z, 0.01) if relu else z)[:, 1:, :])
    rows = torch.cat(rows, dim=1)
    (rows * d_rows.detach().cpu().to(dtype)).sum().backward()
    return rows.detach(), [t.grad for t in ts], [w.grad for w in ws], zmin
