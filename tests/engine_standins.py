"""torch definitions, on the CPU, of the engine calls the IQM branch makes (model/iqm.py, AdaptedCLIP._iqm_branch): what
the host-side tests put in place of the library to check the algebra and the order of calls without a GPU.
install(monkeypatch, counts) replaces them on aaclip_hip.engine; with a dict it counts the calls per function."""
import math

import torch

from aaclip_hip import _lib, engine


def gemm(code, epi, a, w, bias, out, act=0):
    y = a.double() @ w.double().t()
    if bias is not None:
        y = y + bias.double()
    if epi == _lib.EPI_BIAS_GELU:
        y = 0.5 * y * (1 + torch.erf(y / math.sqrt(2)))
    if act == _lib.ACT_RELU:
        y = y.clamp_min(0)
    elif act == _lib.ACT_LEAKY:
        y = torch.where(y > 0, y, 0.01 * y)
    out.copy_(y.to(out.dtype))
    return out


class Cache:
    def get(self, w, code, kind=None):
        w = w.detach().float()
        return w.t().contiguous() if kind == "transpose" else w


def head_expand(q, H, scale, code):
    rows, D = q.shape
    hd = D // H
    out = torch.zeros(rows, H, D)
    for h in range(H):
        out[:, h, h * hd:(h + 1) * hd] = q[:, h * hd:(h + 1) * hd] * scale
    return out.view(rows * H, D)


def head_diag(full, H):
    rows, D = full.shape[0] // H, full.shape[1]
    hd = D // H
    f = full.view(rows, H, D)
    return torch.cat([f[:, h, h * hd:(h + 1) * hd] for h in range(H)], 1).contiguous()


def cross_rows(qt, x, B, R, Lk, code):
    Dk = x.shape[-1]
    p = torch.softmax(qt.double().view(B, R, Dk) @ x.double().view(B, Lk, Dk).transpose(1, 2), -1)
    return (p @ x.double().view(B, Lk, Dk)).float().view(B * R, Dk)


def cross_rows_levels(qt, levels, B, R, rpi, row0, Lk, Dk):
    n = len(levels)
    q = qt.double().view(B, R, n, Dk)
    keys = [x.double().view(B, rpi, -1)[:, row0:row0 + Lk, :Dk] for x in levels]
    p = torch.softmax(torch.cat([torch.einsum("brd,bjd->brj", q[:, :, s], keys[s]) for s in range(n)], -1), -1)
    out = torch.stack([torch.einsum("brj,bjd->brd", p[:, :, s * Lk:(s + 1) * Lk], keys[s]) for s in range(n)], 2)
    return out.float().reshape(B * R, n * Dk)


def small_attention(q, k, v, B, nq, Lk, H, code):
    D = q.shape[-1]
    hd = D // H
    qh = q.double().view(B, nq, H, hd).transpose(1, 2)
    kh = k.double().view(B, Lk, H, hd).transpose(1, 2)
    vh = v.double().view(B, Lk, H, hd).transpose(1, 2)
    return (torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(hd), -1) @ vh).transpose(1, 2).reshape(B * nq, D).float()


def residual_layernorm(a, b, ln, eps):
    x = a if b is None else a + b
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), ln.weight, ln.bias, eps)


def combine3(a, b, c, wa, wb, wc):
    out = wa * a
    for t, w in ((b, wb), (c, wc)):
        if t is not None:
            out = out + w * t
    return out


def linear_smallk(x, weight, bias, out_code):
    y = x.float().reshape(-1, x.shape[-1]) @ weight.float().t()
    return (y if bias is None else y + bias.float()).to(engine.torch_dtype(out_code))


def require_gpu(t, what):
    pass


LAUNCHES = ("gemm", "head_expand", "head_diag", "cross_rows", "cross_rows_levels", "small_attention",
            "residual_layernorm", "combine3", "linear_smallk")


def install(monkeypatch, counts=None):
    """Put the stand-ins on aaclip_hip.engine.  counts (a dict): counts[name] += 1 on every call of a LAUNCHES function
    (and of require_gpu); names that are never called are absent."""
    def counted(name, fn):
        def call(*args, **kwargs):
            counts[name] = counts.get(name, 0) + 1
            return fn(*args, **kwargs)
        return fn if counts is None else call

    monkeypatch.setattr(engine, "CACHE", Cache())
    for name in LAUNCHES + ("require_gpu",):
        monkeypatch.setattr(engine, name, counted(name, globals()[name]))
