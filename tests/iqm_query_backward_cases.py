"""Seeded cases and fp64 torch references shared by tests/test_iqm_query_backward_cpu.py and
tests/test_gpu_iqm_query_backward.py: the entry points of csrc/iqm_query_backward.hip (aaclip_small_attention_backward,
aaclip_layernorm_param_grad, aaclip_bias_grad, aaclip_act_backward, aaclip_linear_smallk_backward).

Every reference is the forward formula differentiated by torch autograd, or the sum itself, in fp64 on the CPU; the same
function in fp32 gives the conditioning figure of a case."""
import functools
import math

import torch
import torch.nn.functional as F

from aaclip_hip import synth

RELU, GELU = 2, 3                        # AACLIP_ACT_RELU, AACLIP_ACT_GELU
MAX_KEYS = 256                           # csrc/kernels.h SAB_MAXK
CHUNK_ROWS, MAX_CHUNKS = 32, 64          # csrc/kernels.h IQB_CHUNK_ROWS, IQB_MAX_CHUNKS


def rnd(name, shape, std=1.0):
    return synth.randn("iqb." + name, shape, std, 47)


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.isfinite(a).all()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------ small_attention_backward
# outs: which of d_q / d_k / d_v the call asks for.  peak: query 0 of every (image, head) is rescaled so that its largest
# scaled score is `peak` above the mean of the others: one key holds the mass.
ATTENTION = {
    "production": dict(B=2, nq=2, Lk=2, H=8, hd=96),
    "one_key": dict(B=1, nq=1, Lk=1, H=1, hd=4),                     # p = 1, ds = 0: d_q and d_k exactly zero
    "crosses_a_wave": dict(B=2, nq=4, Lk=65, H=3, hd=32),
    "upper_edges": dict(B=2, nq=3, Lk=256, H=2, hd=128),
    "peaked_row": dict(B=2, nq=2, Lk=40, H=4, hd=32, peak=60.0),
    "d_q_only": dict(B=2, nq=2, Lk=9, H=4, hd=32, outs=("d_q",)),
    "d_k_only": dict(B=2, nq=2, Lk=9, H=4, hd=32, outs=("d_k",)),
    "d_v_only": dict(B=2, nq=2, Lk=9, H=4, hd=32, outs=("d_v",)),
}


def attention_inputs(name):
    c = ATTENTION[name]
    B, nq, Lk, H, hd = c["B"], c["nq"], c["Lk"], c["H"], c["hd"]
    D = H * hd
    t = {"q": rnd(name + ".q", (B * nq, D)), "k": rnd(name + ".k", (B * Lk, D)), "v": rnd(name + ".v", (B * Lk, D)),
         "d_out": rnd(name + ".d_out", (B * nq, D))}
    if c.get("peak") is not None:
        q4 = t["q"].double().view(B, nq, H, hd)
        k4 = t["k"].double().view(B, Lk, H, hd)
        s = torch.einsum("bqhd,bkhd->bhqk", q4, k4) / math.sqrt(hd)
        f = c["peak"] / s[:, :, 0, :].amax(dim=-1)                    # [B, H]
        q4 = q4.clone()
        q4[:, 0] = q4[:, 0] * f.unsqueeze(-1)
        t["q"] = q4.reshape(B * nq, D).float()
    return t


def attention_reference(t, c, dtype=torch.float64):
    """-> {d_q, d_k, d_v, out} of softmax(q k^T / sqrt(hd)) v per (image, head), in `dtype` on the CPU"""
    B, nq, Lk, H, hd = c["B"], c["nq"], c["Lk"], c["H"], c["hd"]
    q = t["q"].to(dtype).view(B, nq, H, hd).requires_grad_(True)
    k = t["k"].to(dtype).view(B, Lk, H, hd).requires_grad_(True)
    v = t["v"].to(dtype).view(B, Lk, H, hd).requires_grad_(True)
    p = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q, k) / math.sqrt(hd), dim=-1)
    out = torch.einsum("bhqk,bkhd->bqhd", p, v)
    out.backward(t["d_out"].to(dtype).view(B, nq, H, hd))
    D = H * hd
    return {"d_q": q.grad.reshape(B * nq, D), "d_k": k.grad.reshape(B * Lk, D), "d_v": v.grad.reshape(B * Lk, D),
            "out": out.detach().reshape(B * nq, D), "p": p.detach()}


@functools.lru_cache(maxsize=None)
def attention_case(name):
    """-> (inputs, fp64 expectations restricted to the outputs the case asks for)"""
    c = ATTENTION[name]
    t = attention_inputs(name)
    ref = attention_reference(t, c)
    outs = c.get("outs", ("d_q", "d_k", "d_v"))
    return t, {k: (ref[k] if k in outs else None) for k in ("d_q", "d_k", "d_v")}


# ------------------------------------------------------------------------------------------ layernorm_param_grad
LAYERNORM = {f"D{D}_rows{rows}_eps{eps:g}": dict(D=D, rows=rows, eps=eps)
             for D, rows, eps in ((256, 1, 1e-12), (256, 4, 1e-5), (768, 4, 1e-12), (768, 5, 1e-5), (768, 130, 1e-12),
                                  (1024, 4, 1e-5), (1024, 130, 1e-5), (256, 5, 1e-12))}


def layernorm_inputs(name):
    c = LAYERNORM[name]
    return {"x": rnd(name + ".x", (c["rows"], c["D"])) + 0.3, "d_y": rnd(name + ".d_y", (c["rows"], c["D"]))}


def layernorm_reference(t, c, dtype=torch.float64):
    D = c["D"]
    w = torch.ones(D, dtype=dtype, requires_grad=True)
    b = torch.zeros(D, dtype=dtype, requires_grad=True)
    F.layer_norm(t["x"].to(dtype), (D,), w, b, c["eps"]).backward(t["d_y"].to(dtype))
    return {"d_w": w.grad, "d_b": b.grad}


@functools.lru_cache(maxsize=None)
def layernorm_case(name):
    t = layernorm_inputs(name)
    return t, layernorm_reference(t, LAYERNORM[name])


# ------------------------------------------------------------------------------------------ bias_grad
# pad: ldz - N columns of NaN behind every row, which the kernel must not read
BIAS = {f"N{N}_rows{rows}" + ("_padded" if pad else ""): dict(N=N, rows=rows, pad=pad)
        for N, rows, pad in ((768, 1, 0), (768, 4, 0), (768, 129, 0), (2048, 1, 0), (2048, 4, 0), (2048, 129, 0),
                             (768, 4, 8), (2048, 129, 4))}


def bias_inputs(name):
    c = BIAS[name]
    dz = torch.full((c["rows"], c["N"] + c["pad"]), float("nan"))
    dz[:, :c["N"]] = rnd(name + ".dz", (c["rows"], c["N"]))
    return {"dz": dz}


def bias_reference(t, c, dtype=torch.float64):
    return {"db": t["dz"][:, :c["N"]].to(dtype).sum(dim=0)}


@functools.lru_cache(maxsize=None)
def bias_case(name):
    t = bias_inputs(name)
    return t, bias_reference(t, BIAS[name])


# ------------------------------------------------------------------------------------------ act_backward
ACT = {f"{'gelu' if act == GELU else 'relu'}_n{n}": dict(act=act, n=n)
       for act in (GELU, RELU) for n in (1, 255, 257, 4096)}


def act_inputs(name):
    """zy: the GELU's pre-activation (with 0 and +-10 among the values), or the ReLU's OUTPUT (exact zeros included)"""
    c = ACT[name]
    n = c["n"]
    z = rnd(name + ".z", (n,), 1.5)
    special = torch.tensor([0.0, 10.0, -10.0])
    if n >= 255:
        z[3:6] = special
        z[n - 1] = 0.0
    else:
        z[0] = 0.0                                 # the single element sits on the kink
    if c["act"] == RELU:
        z = torch.relu(z)
    return {"zy": z, "d_y": rnd(name + ".d_y", (n,))}


def act_reference(t, c, dtype=torch.float64):
    z, g = t["zy"].to(dtype), t["d_y"].to(dtype)
    if c["act"] == GELU:
        z = z.clone().requires_grad_(True)
        F.gelu(z).backward(g)                      # the erf form
        return {"d_z": z.grad}
    return {"d_z": torch.where(z > 0, g, torch.zeros((), dtype=dtype))}


@functools.lru_cache(maxsize=None)
def act_case(name):
    t = act_inputs(name)
    return t, act_reference(t, ACT[name])


# ------------------------------------------------------------------------------------------ linear_smallk_backward
SMALLK = {f"R{R}_N{N}_K{K}": dict(R=R, N=N, K=K)
          for R, N, K in ((1, 64, 1), (768, 768, 2), (2 * 768 + 3, 768, 2), (300, 64, 4))}


def smallk_inputs(name):
    c = SMALLK[name]
    return {"x": rnd(name + ".x", (c["R"], c["K"])), "d_y": rnd(name + ".d_y", (c["R"], c["N"]))}


def smallk_reference(t, c, dtype=torch.float64):
    w = torch.zeros(c["N"], c["K"], dtype=dtype, requires_grad=True)
    b = torch.zeros(c["N"], dtype=dtype, requires_grad=True)
    F.linear(t["x"].to(dtype), w, b).backward(t["d_y"].to(dtype))
    return {"d_w": w.grad, "d_b": b.grad}


@functools.lru_cache(maxsize=None)
def smallk_case(name):
    t = smallk_inputs(name)
    return t, smallk_reference(t, SMALLK[name])


# entry -> (case table, inputs, reference(t, c, dtype), cached case)
ENTRIES = {
    "small_attention_backward": (ATTENTION, attention_inputs, attention_reference, attention_case),
    "layernorm_param_grad": (LAYERNORM, layernorm_inputs, layernorm_reference, layernorm_case),
    "bias_grad": (BIAS, bias_inputs, bias_reference, bias_case),
    "act_backward": (ACT, act_inputs, act_reference, act_case),
    "linear_smallk_backward": (SMALLK, smallk_inputs, smallk_reference, smallk_case),
}
ALL_CASES = [(e, n) for e, v in ENTRIES.items() for n in v[0]]


def chunks_of(rows):
    """chunk count of the column sums (csrc/iqm_query_backward.hip iqb_chunks)"""
    return min(MAX_CHUNKS, -(-rows // CHUNK_ROWS))
