"""The block path's fused GEMM epilogues and e4m3 attention records (include/aaclip.h, "The block path's forms of the
building blocks"): host builders, a torch emulation of the folded arithmetic and the cases shared by
tests/test_fused_epilogues_cpu.py and tests/test_gpu_fused_epilogues.py.

LayerNorm folding replaces y = LN(x) . W^T + bias by

    x16 = round16(x);  (sum, sumsq) per 64-column slice of x16 in fp32;  mean = S / D,  var = max(Q / D - mean^2, 0)
    (a, b) = (rstd, -mean * rstd);  y = fmaf(a, x16 . (W gamma)^T, b * s) + (bias + W beta),  s = row sums of round16(W gamma)

The ONE-PASS variance cancels on rows with a large common mean: the relative error of rstd tracks 2^-24 kappa with
kappa = mean(x^2) / (var + eps).  The emulation below reproduces that arithmetic in fp32 (not the kernel's summation
order), so it tells what the form costs on a row kind before any kernel runs, and the GPU tests take their bars for the
cancelling kinds from it."""
import functools

import torch

from aaclip_hip import engine, synth

EPS = 1e-5
WIDTHS = (256, 768, 1024)
KINDS = ("plain", "mean8", "mean30", "outlier", "tiny", "constant")
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
ET = {"fp16": 1.5e-3, "bf16": 1.2e-2}               # tests/test_gpu_parity.py test_gemm_epilogues: output rounding
RSTD_BOUND = 8 * 2.0 ** -24                          # times kappa: relative error of rstd (the emulation, D = 1024, fp16
                                                     # rows: 2e-7 plain, 7e-6 at mean 8, 2.8e-4 at mean 30, 1e-3 at mean 100)
FIN_ROWS = (1, 15, 16, 17, 4097)                     # 16 lanes per row, 256 threads per workgroup
GEMM_ROWS = (4096, 4097, 4225)                       # 4225: last tile = one full 128-row band + a band of one row


def rows(kind, M, D, seed=0):
    """fp32 [M, D] residual rows of one kind (deterministic)"""
    g = torch.Generator().manual_seed(1000 * seed + 10 * D + KINDS.index(kind))
    z = torch.randn(M, D, generator=g)
    if kind == "plain":
        return 0.7 + 3.0 * z
    if kind == "mean8":
        return 8.0 + z
    if kind == "mean30":
        return 30.0 + 0.5 * z
    if kind == "outlier":
        x = 0.7 + 3.0 * z
        x[torch.arange(M), torch.randint(0, D, (M,), generator=g)] += 300.0
        return x
    if kind == "tiny":
        return 1e-3 * z
    if kind == "constant":
        return torch.full((M, D), 2.5)
    raise KeyError(kind)


def round16(x, dtype):
    """fp32 -> the 16-bit format and back (fp32 tensor holding 16-bit values)"""
    return x.float().to(TDT[dtype]).float()


def slice_stats64(x16):
    """fp64 (sum, sumsq) per 64-column slice of 16-bit values -> [M, D / 64, 2], and the magnitudes (sum |r|, sum r^2)
    that scale the fp32 summation error of a slot"""
    v = x16.double().reshape(x16.shape[0], -1, 64)
    return torch.stack([v.sum(-1), (v * v).sum(-1)], -1), torch.stack([v.abs().sum(-1), (v * v).sum(-1)], -1)


def slice_stats_emulated(x16):
    """the same sums in fp32 -> fp32 [M, D / 64, 2] (what stats_out holds, up to the order of the 64 terms)"""
    v = x16.float().reshape(x16.shape[0], -1, 64)
    return torch.stack([v.sum(-1), (v * v).sum(-1)], -1).contiguous()


def finalize_emulated(partials, D, eps=EPS):
    """fp32 partials [M, slots, 2] -> fp32 [M, 2] = (rstd, -mean * rstd), one-pass variance as the kernels take it"""
    p = partials.float()
    inv_d = torch.tensor(1.0 / D, dtype=torch.float32)
    s, q = p[:, :, 0].sum(1), p[:, :, 1].sum(1)
    mean = s * inv_d
    var = (q * inv_d - mean * mean).clamp_min(0.0)
    rstd = torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32))
    return torch.stack([rstd, -mean * rstd], 1).contiguous()


def finalize64(partials, D, eps=EPS):
    """fp64 (rstd, -mean * rstd) and kappa = mean(x^2) / (var + eps) of the SAME partials"""
    p = partials.double()
    s, q = p[:, :, 0].sum(1), p[:, :, 1].sum(1)
    mean = s / D
    var = (q / D - mean * mean).clamp_min(0.0)
    rstd = (var + eps).rsqrt()
    return torch.stack([rstd, -mean * rstd], 1), (q / D) / (var + eps)


def ab_bounds(ab64, kappa):
    """allowed |error| of (rstd, b) per row.  rstd: RSTD_BOUND * kappa relative (the cancellation of q / D - mean^2; at
    least one plain fp32 rounding chain, so kappa counts as >= 1).  b = -mean * rstd inherits that relative error, plus
    the fp32 error of the mean itself scaled by rstd: |d mean| rstd <= c 2^-24 mean|x| rstd <= c 2^-24 sqrt(kappa), so
    the scale of b's bound is max(|b|, 1) -- absolute where the mean is near zero."""
    k = kappa.clamp_min(1.0)
    return torch.stack([RSTD_BOUND * k * ab64[:, 0], RSTD_BOUND * k * ab64[:, 1].abs().clamp_min(1.0)], 1)


def fmaf32(a, x, c):
    """fp32 fmaf(a, x, c): the product of two fp32 values is exact in fp64"""
    return (a.double() * x.double() + c.double()).float()


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def fold_weights(W, bias, gamma, beta, dtype):
    """engine.FoldCache._fold on fp32 parameters -> (W gamma in 16 bits, its fp32 row sums, bias + W beta)"""
    wf = (W.float() * gamma.float()[None, :]).to(TDT[dtype]).contiguous()
    return wf, wf.float().sum(dim=1).contiguous(), (bias.float() + W.float() @ beta.float()).contiguous()


def folded_emulated(x16, ab, wf, col_s, fbias, gelu):
    """fp32 emulation of the folded epilogue on 16-bit rows x16 (fp32 tensor) -> fp32 values before the output rounding"""
    acc = x16.float() @ wf.float().t()
    v = fmaf32(ab[:, :1], acc, ab[:, 1:2] * col_s[None, :].float()) + fbias[None, :].float()
    return gelu64(v.double()).float() if gelu else v


def chain_reference64(x16, W, bias, gamma, beta, gelu):
    """fp64 act(LN(x16) W^T + bias) on the 16-bit rows, with the two-pass variance"""
    x = x16.double()
    y = torch.nn.functional.layer_norm(x, (x.shape[1],), gamma.double(), beta.double(), EPS)
    v = y @ W.double().t() + bias.double()
    return gelu64(v) if gelu else v


@functools.lru_cache(maxsize=None)
def chain_params(D, N):
    """LayerNorm and Linear parameters of the chain cases: gamma about 1, beta and bias about 0.2, W ~ D^-1/2"""
    return (synth.randn(f"fused.chain.w.{D}.{N}", (N, D), D ** -0.5, 11), synth.randn(f"fused.chain.b.{N}", (N,), 0.2, 11),
            synth.randn(f"fused.chain.g.{D}", (D,), 0.2, 11, 1.0), synth.randn(f"fused.chain.be.{D}", (D,), 0.2, 11))


# ---- e4m3 attention records: [q k v hi: 3D fp16][q: per head lo8 64 B | hi8 64 B][k: the same], 10 D bytes per row
def qk8_records_cols(x, out_qk8):
    """fp32 [R, N] -> uint8 [R, 2 N + 2 out_qk8]: the out_qk8 row of aaclip_gemm_fused -- engine.split_rows' fp16 plane,
    then per 64 columns below out_qk8 that group's [lo8 64 B | hi8 64 B]"""
    R, N = x.shape
    s = engine.split_rows(x)
    hi, lo8, hi8 = s[:, :2 * N], s[:, 2 * N:3 * N], s[:, 3 * N:4 * N]
    G = out_qk8 // 64
    rec = torch.stack([lo8[:, :out_qk8].reshape(R, G, 64), hi8[:, :out_qk8].reshape(R, G, 64)], 2)
    return torch.cat([hi, rec.reshape(R, 2 * out_qk8)], 1).contiguous()


def qk8_records(qkv, H):
    """fp32 q|k|v [R, 3 * 64 H] -> uint8 [R, 10 * 64 H]: engine.split_rows' planes rearranged per head (v keeps its fp16
    half only)"""
    return qk8_records_cols(qkv, 128 * H)


def qk8_planes(rec, H):
    """records -> (hi fp16 [R, 3D], lo8 bytes [R, 2D], hi8 bytes [R, 2D])"""
    D = 64 * H
    b = rec.contiguous().view(torch.uint8).reshape(rec.shape[0], -1).cpu()
    assert b.shape[1] == 10 * D, (b.shape, D)
    r = b[:, 6 * D:].reshape(-1, 2 * H, 2, 64)
    return (b[:, :6 * D].contiguous().view(torch.float16), r[:, :, 0].reshape(-1, 2 * D).contiguous(),
            r[:, :, 1].reshape(-1, 2 * D).contiguous())


def qk8_join(rec, H):
    """records -> fp64 [R, 3D]: hi + lo8 * 2^-10 for q and k, hi for v (what the attention kernel sees)"""
    D = 64 * H
    hi, lo8, _ = qk8_planes(rec, H)
    out = hi.double()
    out[:, :2 * D] += lo8.view(torch.float8_e4m3fn).double() / float(2 ** engine.SPLIT8_ACT_LO_EXP)
    return out


def qk8_without_corrections(rec, H):
    """the same records with every e4m3 byte zero: fp16 q and k"""
    out = rec.clone()
    out[:, 6 * 64 * H:] = 0
    return out


QK8_ATTENTION_CASES = [(1, 1, 512), (1, 1, 513), (1, 2, 576), (3, 1, 513)]      # B, H, L; non-causal, q in log2 units


def attention_inputs(B, H, L):
    """fp32 q|k|v [B * L, 3 * 64 H], q in log2 units (tests/test_gpu_split.py test_attention_split's draw)"""
    qkv = synth.randn(f"fused.attn.{B}.{H}.{L}", (B * L, 192 * H), 1.0, 3)
    qkv[:, :64 * H] *= 0.6 * 1.4426950408889634
    return qkv


def attention_reference64(qkv_seen, B, L, H):
    """fp64 softmax(q k^T) v of the values the kernel sees (q in log2 units)"""
    D = 64 * H
    f = qkv_seen.double().clone()
    f[:, :D] *= 0.6931471805599453
    q, k, v = f.view(B, L, 3, H, 64).permute(2, 0, 3, 1, 4)
    return (torch.softmax(q @ k.transpose(-1, -2), -1) @ v).transpose(1, 2).reshape(B * L, D)
