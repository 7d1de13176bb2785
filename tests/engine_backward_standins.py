"""torch definitions, on the CPU, of the BACKWARD engine calls the IQM branch's training routes make
(aaclip_hip/autograd.py: _iqm_query_walk, IqmQueries, IqmQueriesFolded): the companion of tests/engine_standins.py for
checking the algebra of a backward route without a GPU.  Plain fp32 in and out, fp64 inside, 16-bit casts the identity.
install(monkeypatch, counts) puts these and the forward stand-ins on aaclip_hip.engine."""
import math

import torch
import torch.nn.functional as F

import engine_standins as SI
from aaclip_hip import _lib, engine


def _grads(outs, d_outs, ins):
    total = sum((o * d.double()).sum() for o, d in zip(outs, d_outs))
    return [g.float() for g in torch.autograd.grad(total, ins)]


def gemm_wgrad(dz, u):
    return (dz.double().t() @ u.double()).float()


def bias_grad(dz, N=None):
    return dz.double()[:, :N].sum(0).float()


def layernorm_param_grad(x, d_y, eps):
    x = x.double().reshape(-1, x.shape[-1])
    xhat = (x - x.mean(-1, keepdim=True)) / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + eps)
    d = d_y.double().reshape(x.shape)
    return (d * xhat).sum(0).float(), d.sum(0).float()


def layernorm_backward(x, weight, d_y, d_resid=None, eps=1e-5):
    with torch.enable_grad():
        xx = x.detach().double().requires_grad_(True)
        y = F.layer_norm(xx, (xx.shape[-1],), weight.detach().double(), None, eps)
        (g,) = _grads([y], [d_y.reshape(y.shape)], [xx])
    return g if d_resid is None else g + d_resid.float()


def small_attention_backward(q, k, v, d_out, B, nq, Lk, heads, need_q=True, need_k=True, need_v=True):
    with torch.enable_grad():
        ins = [t.detach().double().requires_grad_(True) for t in (q, k, v)]
        D = q.shape[-1]
        hd = D // heads
        qh, kh, vh = (t.view(B, n, heads, hd).transpose(1, 2) for t, n in zip(ins, (nq, Lk, Lk)))
        out = (torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(hd), -1) @ vh).transpose(1, 2).reshape(B * nq, D)
        g = _grads([out], [d_out.reshape(out.shape)], ins)
    return tuple(t if need else None for t, need in zip(g, (need_q, need_k, need_v)))


def cross_rows_backward(qt, x, d_out, B, R, Lk, x_code, act=_lib.ACT_NONE, need_qt=True, need_x=True, d_x=None):
    assert act == _lib.ACT_NONE
    with torch.enable_grad():
        Dk = x.shape[-1]
        q = qt.detach().double().view(B, R, Dk).requires_grad_(True)
        xx = x.detach().double().view(B, Lk, Dk).requires_grad_(True)
        out = torch.softmax(q @ xx.transpose(1, 2), -1) @ xx
        g_q, g_x = _grads([out], [d_out.reshape(out.shape)], [q, xx])
    g_x = g_x.reshape(B * Lk, Dk)
    if need_x and d_x is not None:
        g_x = d_x.add_(g_x)
    return (g_q.reshape(B * R, Dk) if need_qt else None), (g_x if need_x else None)


def cross_rows_levels_backward(qt, levels, d_out, B, R, rpi, row0, Lk, Dk, need_qt=True, need_x=True, d_x=None,
                               overwrite=False):
    n = len(levels)
    with torch.enable_grad():
        q = qt.detach().double().view(B, R, n, Dk).requires_grad_(True)
        keys = [x.detach().double().view(B, rpi, -1)[:, row0:row0 + Lk, :Dk].contiguous().requires_grad_(True)
                for x in levels]
        p = torch.softmax(torch.cat([torch.einsum("brd,bjd->brj", q[:, :, s], keys[s]) for s in range(n)], -1), -1)
        out = torch.stack([torch.einsum("brj,bjd->brd", p[:, :, s * Lk:(s + 1) * Lk], keys[s]) for s in range(n)], 2)
        g = _grads([out], [d_out.reshape(out.shape)], [q] + keys)
    if need_x:
        if d_x is None:
            d_x = [torch.zeros(B * rpi, Dk) for _ in range(n)]
        for buf, gk in zip(d_x, g[1:]):
            rows = buf.view(B, rpi, Dk)[:, row0:row0 + Lk]
            rows.copy_(gk if overwrite else rows + gk)
    return (g[0].reshape(B * R, n * Dk) if need_qt else None), (list(d_x) if need_x else None)


def act_backward(act, zy, d_y, in_place=False):
    z = zy.double().reshape(d_y.shape)
    if act == _lib.ACT_GELU:
        slope = 0.5 * (1 + torch.erf(z / math.sqrt(2))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
    else:
        assert act == _lib.ACT_RELU
        slope = (z > 0).double()
    d_z = (d_y.double() * slope).float()
    return d_y.copy_(d_z) if in_place else d_z


def linear_smallk_backward(x, d_y):
    K = x.shape[-1]
    return (d_y.double().t() @ x.double().reshape(-1, K)).float(), d_y.double().sum(0).float()


LAUNCHES = ("gemm_wgrad", "bias_grad", "layernorm_param_grad", "layernorm_backward", "small_attention_backward",
            "cross_rows_backward", "cross_rows_levels_backward", "act_backward", "linear_smallk_backward")


def install(monkeypatch, counts=None):
    """The forward stand-ins (engine_standins.install) plus the backward ones above; counts as there."""
    SI.install(monkeypatch, counts)

    def counted(name, fn):
        def call(*args, **kwargs):
            counts[name] = counts.get(name, 0) + 1
            return fn(*args, **kwargs)
        return fn if counts is None else call

    for name in LAUNCHES:
        monkeypatch.setattr(engine, name, counted(name, globals()[name]))
