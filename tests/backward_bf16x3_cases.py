"""The bf16x3 backward of the visual blocks (include/aaclip.h "bf16x3"): a torch emulation of its arithmetic and the
cases shared by tests/test_backward_bf16x3_cpu.py and tests/test_gpu_backward_bf16x3.py.

The emulation carries a value as hi = bf16(v), lo = bf16(v - hi) and sums a product as Ah.Bh + Al.Bh + Ah.Bl in fp32;
everything else (softmax statistics, exponent, ds) is fp32, as in the kernels.  It tells what the arithmetic costs on a
case before any kernel runs: the bar of the GPU tests (1e-4 relative Frobenius against fp64, the bar of
tests/test_gpu_visual_backward.py) must hold for the emulation with room, or the case is a bad case."""
import functools

import torch

import oracle.aaclip_oracle as O
import visual_backward_cases as VB
from aaclip_hip import synth
from visual_backward_cases import attention_inputs, attention_reference, build_clip, rel, rnd  # noqa: F401

BAR = 1e-4

# VB.ATTENTION_CASES without (2, 4, 128) and (1, 4, 256): they repeat the tile situations of (2, 4, 160) / (2, 16, 257)
ATTENTION_CASES = [(1, 1, 1), (2, 4, 31), (1, 2, 32), (3, 4, 77), (1, 1, 129), (2, 4, 160), (2, 16, 257), (1, 2, 1370)]
PEAKED = (2, 4, 257, 30.0)            # B, H, L, largest score of every row; image 1's d_ctx is zero
RANGE = (2, 4, 160, 2.0 ** -40)       # B, H, L, factor on d_ctx: fp16 operands would flush these gradients to zero
SPLIT_SHAPES = [(1, 64), (33, 256), (3, 4096), (170, 1024)]

# name -> (width, B, L, causal): the drawn inputs of tests/test_gpu_visual_backward.py's cases of the same name, no adapter
PLAIN_BLOCK_CASES = {
    "visual_length_reduced_width": ("tiny", 1, 1370, False),
    "causal": ("tiny", 2, 160, True),
    "full_width_plain": ("full", 2, 170, False),
}
# The one adapter case: tiny width, one row into the second 32-row tile.  The gradient is discontinuous where an adapter
# pre-activation z is 0 (LeakyReLU; VB.BLOCK_CASES says what one flipped element costs), and this mode's recomputed z is
# off by about 2e-5 of its rms, so the case must keep min|z| well above that: Z_CLEARANCE (asserted in the CPU file).
ADAPTER_CASE = dict(width="tiny", B=1, L=33, mix=0.1, x_name="bf16x3.blk.x.adapter.284", do_name="bf16x3.blk.do.adapter")
Z_CLEARANCE = 5e-4                    # min|z| / rms(z), in fp64


def split(x):
    """fp32 -> (hi, lo) as fp32 tensors holding bf16 values"""
    x = x.float()
    hi = x.bfloat16()
    return hi.float(), (x - hi.float()).bfloat16().float()


def mm3(a, b):
    """a @ b in three terms, fp32 sums"""
    ah, al = split(a)
    bh, bl = split(b)
    return al @ bh + ah @ bl + ah @ bh


def attention_backward_emulated(qkv, d_ctx, B, H, L, causal):
    """d qkv [B*L, 3*64*H] of softmax(q k^T) v in the kernels' arithmetic (q pre-scaled)"""
    D = 64 * H
    q, k, v = (t.float().reshape(B, L, H, 64).transpose(1, 2) for t in qkv.split(D, dim=-1))
    d = d_ctx.float().reshape(B, L, H, 64).transpose(1, 2)
    s = mm3(q, k.transpose(-1, -2))
    if causal:
        s = s + O.causal_mask(L, torch.float32)
    p = torch.softmax(s, dim=-1)
    dp = mm3(d, v.transpose(-1, -2))
    ds = p * (dp - (p * dp).sum(dim=-1, keepdim=True))
    dq, dk, dv = mm3(ds, k), mm3(ds.transpose(-1, -2), q), mm3(p.transpose(-1, -2), d)
    return torch.cat([t.transpose(1, 2).reshape(B * L, D) for t in (dq, dk, dv)], dim=-1)


def attention_errors(got, want, H, rows=None):
    D = 64 * H
    g, w = (got, want) if rows is None else (got[:rows], want[:rows])
    return {"dq": rel(g[:, :D], w[:, :D]), "dk": rel(g[:, D:2 * D], w[:, D:2 * D]), "dv": rel(g[:, 2 * D:], w[:, 2 * D:]),
            "all": rel(g, w)}


@functools.lru_cache(maxsize=None)
def peaked_case():
    """-> (qkv, d_ctx, fp64 d qkv) of PEAKED"""
    B, H, L, peak = PEAKED
    qkv, d_ctx = attention_inputs(B, H, L, peak=peak)
    d_ctx[L:] = 0
    return qkv, d_ctx, attention_reference(qkv, d_ctx, B, H, L, False)


@functools.lru_cache(maxsize=None)
def range_case():
    """-> (qkv, scaled d_ctx, fp64 d qkv of the scaled input) of RANGE"""
    B, H, L, factor = RANGE
    qkv, d_ctx, _ = VB.attention_case(B, H, L, False)
    small = d_ctx * factor          # a power of two: exact
    return qkv, small, attention_reference(qkv, small, B, H, L, False)


def split_inputs(rows, K):
    """N(0, 1), the same times 2^-40 and 2^40, with one row of zeros each -> [(name, fp32 [rows, K])]"""
    x = rnd(f"bf16x3.split.{rows}.{K}", (rows, K))
    out = []
    for name, f in (("unit", 1.0), ("tiny", 2.0 ** -40), ("huge", 2.0 ** 40)):
        y = x * f
        y[rows // 2] = 0
        out.append((name, y))
    return out


def split_planes(x):
    """the three planes [hi | lo | hi] torch gives for x, bf16 [rows, 3K]"""
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    return torch.cat([hi, lo, hi], dim=1)


def block_cfg(width):
    return synth.tiny_cfg() if width == "tiny" else VB.full_width_cfg()


def block_reference(sd, cfg, x, d_out, B, L, causal, aw=None, mix=0.0):
    """fp64 autograd of resblocks.0 (+ adapter mix) -> (d x [B*L, D], d adapter weight or None, z or None)"""
    D, H = cfg.vision.width, cfg.vision.heads
    pre = "visual.transformer.resblocks.0."
    sd64 = {k: v.double() for k, v in sd.items() if k.startswith(pre)}
    x64 = x.double().reshape(B, L, D).requires_grad_(True)
    y = O.resblock(x64, sd64, pre, H, O.causal_mask(L, torch.float64) if causal else None)
    a64, z = None, None
    if aw is not None:
        a64 = aw.double().requires_grad_(True)
        z = (y @ a64.t()).detach()
        y = O.adapter_mix(y, a64, mix)
    y.backward(d_out.double().reshape(B, L, D))
    return x64.grad.reshape(B * L, D), None if a64 is None else a64.grad, z


@functools.lru_cache(maxsize=None)
def adapter_case():
    """-> (cfg, sd, x, d_out, adapter weight, fp64 d x, fp64 d adapter weight, fp64 z) of ADAPTER_CASE"""
    c = ADAPTER_CASE
    cfg = block_cfg(c["width"])
    sd, _ = build_clip(cfg, "fp32", 7)
    D = cfg.vision.width
    x = rnd(c["x_name"], (c["B"] * c["L"], D))
    d_out = rnd(c["do_name"], (c["B"] * c["L"], D))
    aw = synth._xavier(f"vb.blk.adapter.{D}", D, D, 29)
    d_x, d_aw, z = block_reference(sd, cfg, x, d_out, c["B"], c["L"], False, aw, c["mix"])
    return cfg, sd, x, d_out, aw, d_x, d_aw, z
