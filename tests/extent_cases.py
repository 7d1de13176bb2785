"""Entry points on operands whose EXTENT passes 2^31 and 2^32 bytes, and at the size limits include/aaclip.h states
(tests/test_gpu_extent.py; pinned on the CPU by tests/test_extent_cases_cpu.py).

A large operand is made without large work: row r of every operand that grows with the row count is base[r % P] with
an odd period P = 1021, gathered on the device.  One fp64 reference of P rows then covers the whole tensor -- every row
kernel here computes a row from that row alone -- and a row offset that wraps at 32 bits lands on a row of another
phase: row 2^20 of an fp32 [rows, 1024] operand has phase 9, and the wrapped offset 0 is row 0.

Checks of a case: (a) rows [0, P) against the fp64 reference at the tolerance of the entry's existing test (named in
the table); (b) every later row r equals row r % P byte for byte; guards of 4 KiB on both sides of every output intact,
and for strided outputs the gap columns.  Reductions over rows are compared with sum_j count_j * term_j in fp64."""
import functools
import os
import re

import numpy as np
import torch

import backward_blocks_cases as BB
import metrics_device_cases as MD
from aaclip_hip import synth

P = 1021                                  # odd and prime: coprime to every power of two
ROWS = 2 ** 20 + 2051                     # fp32 [ROWS, 1024]: 4 GiB + 8 MiB
WIDTH = 1024
LIMITS = (1 << 31, 1 << 32)
F32, F16, BF16, F16X2 = 0, 1, 2, 3        # AACLIP_F32 ...
EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESID, EPI_ACT_F32 = 0, 1, 2, 3
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPI = os.path.join(REPO, "aa-clip-iqm_amd", "csrc", "capi.hip")


def rnd(name, shape, std=1.0, mean=0.0):
    return synth.randn("extent." + name, shape, std, 61, mean)


# ------------------------------------------------------------------------------------------------ period and crossings
def counts(rows, period=P):
    """count_j = how many rows r < rows have r % period == j (int64 [period])"""
    j = np.arange(period, dtype=np.int64)
    return rows // period + (j < rows % period).astype(np.int64)


def crossings(rows, row_bytes):
    """-> {limit: row}: for each of 2^31 and 2^32 that the operand's byte extent rows * row_bytes passes, the row that
    holds (or starts at) that byte"""
    return {lim: lim // row_bytes for lim in LIMITS if rows * row_bytes > lim}


def wrapped_offset(offset, bits=32, signed=False):
    """what a 64-bit offset becomes when it is truncated to `bits` bits (and sign-extended back when signed)"""
    v = offset & ((1 << bits) - 1)
    if signed and v >> (bits - 1):
        v -= 1 << bits
    return v


def ragged(rows):
    return all(rows % m for m in (4, 128, 256, P))


class Operand:
    """name, role ('in', 'out' or 'inout'), bytes per row (the row stride for a strided operand), fp32 or not, and
    whether it scales with the row count through a row wide enough to reach the limits (`narrow`: a few bytes per row,
    such as the (rstd, b) pairs, which no permitted row count brings to 2^31)"""
    def __init__(self, name, role, row_bytes, fp32, narrow=False):
        self.name, self.role, self.row_bytes, self.fp32, self.narrow = name, role, row_bytes, fp32, narrow


def op(name, role, row_bytes, fp32, narrow=False):
    return Operand(name, role, row_bytes, fp32, narrow)


# ------------------------------------------------------------------------------------------------ group 1: row entries
# name -> (rows, operands, existing test whose tolerance check (a) uses)
_F, _H = 4 * WIDTH, 2 * WIDTH
HEAD_H = 16
HEAD_ROWS = 2 ** 16 + 37                  # just past the row count at which the expanded fp32 operand reaches 2^32 bytes
# a launch covers its grid below 2^24 workgroups of 256 threads only (csrc/capi.hip grid_fits): the entries that take
# one workgroup per 4 rows allow rows <= ROWS4_MAX, one per row < GRID_MAX
GRID_MAX = 1 << 24
ROWS4_MAX = 4 * (GRID_MAX - 1)
ROWS4_REFUSED = ROWS4_MAX + 1
HEAD_MAX_ROWS, HEAD_MAX_D = (GRID_MAX - 1) // 3, 384      # H = 3 heads of 128: rows * H = 2^24 - 1 exactly
ROW_CASES = {
    "layernorm_f32": (ROWS, [op("x", "in", _F, True), op("out", "out", _F, True)],
                      "tests/test_gpu_parity.py test_layernorm: 2e-6 + 1e-5 |ref|"),
    "layernorm_f16": (ROWS, [op("x", "in", _F, True), op("out", "out", _H, False)],
                      "tests/test_gpu_parity.py test_layernorm: 2e-3 + 1e-2 |ref|"),
    "layernorm_bf16": (ROWS, [op("x", "in", _F, True), op("out", "out", _H, False)],
                       "tests/test_gpu_parity.py test_layernorm: 2e-2 + 1e-2 |ref|"),
    "layernorm_split_hi8": (ROWS, [op("x", "in", _F, True), op("out", "out", _F, False)],
                            "tests/test_gpu_split.py test_layernorm_split_output: 6e-6 + 2^-14 |ref| on hi + lo8"),
    "layernorm_split_no_hi8": (ROWS, [op("x", "in", _F, True), op("out", "out", _F, False)],
                               "tests/test_gpu_split.py test_layernorm_split_output: 6e-6 + 2^-14 |ref| on hi + lo8"),
    "split_rows": (ROWS, [op("src", "in", _F, True), op("dst", "out", _F, False)],
                   "tests/test_gpu_fused_epilogues.py test_layernorm_and_split_rows_without_hi8: engine.split_rows' bytes"),
    "split3_rows": (ROWS, [op("src", "in", _F, True), op("dst", "out", 6 * WIDTH, False)],
                    "tests/test_gpu_backward_bf16x3.py test_split3_rows_bit_for_bit: split_planes' bits"),
    "adapter_mix": (ROWS, [op("x", "inout", _F, True), op("a", "in", _F, True)],
                    "tests/test_gpu_parity.py test_adapter_mix: 1e-5 + 1e-5 |ref|"),
    "adapter_mix_fold_f16": (ROWS, [op("x", "inout", _F, True), op("a", "in", _F, True), op("out16", "out", _H, False),
                                    op("row_ab", "out", 8, True, narrow=True)],
                             "tests/test_gpu_fused_epilogues.py: x equals aaclip_adapter_mix's bits, out16 its rounding, "
                             "row_ab within FC.ab_bounds"),
    "residual_layernorm": (ROWS, [op("a", "in", _F, True), op("b", "in", _F, True), op("out", "out", _F, True)],
                           "tests/test_gpu_iqm.py test_residual_layernorm_combine_smallk_dropcls: 1e-5 + 1e-5 |ref|"),
    "combine3": (ROWS, [op("a", "in", _F, True), op("b", "in", _F, True), op("c", "in", _F, True),
                        op("out", "out", _F, True)],
                 "tests/test_gpu_iqm.py test_residual_layernorm_combine_smallk_dropcls: 1e-6 + 1e-6 |ref|"),
    "layernorm_backward": (ROWS, [op("x", "in", _F, True), op("d_y", "in", _F, True), op("d_resid", "in", _F, True),
                                  op("d_x", "out", _F, True)],
                           "tests/test_gpu_backward_blocks.py test_layernorm_backward_per_element: BB.LN_K 2^-24 terms"),
    "adapter_mix_backward": (ROWS, [op("u", "in", _F, True), op("z", "in", _F, True), op("d_y", "in", _F, True),
                                    op("d_z", "out", _F, True), op("d_u", "out", _F, True)],
                             "tests/test_gpu_backward_blocks.py test_adapter_mix_backward_per_element: BB.MIX_K 2^-24 terms"),
    "act_backward_gelu": (ROWS, [op("zy", "in", _F, True), op("d_y", "in", _F, True), op("d_z", "out", _F, True)],
                          "tests/test_gpu_iqm_query_backward.py test_entry_against_fp64: relative Frobenius 1e-4"),
    "act_backward_relu": (ROWS, [op("zy", "in", _F, True), op("d_y", "in", _F, True), op("d_z", "out", _F, True)],
                          "tests/test_gpu_iqm_query_backward.py test_entry_against_fp64: relative Frobenius 1e-4"),
    # 128 bytes of partials per row: only the entry's own limit, rows = 2^27 - 1, brings them past 2^32 (16 GiB - 128)
    "ln_stats_finalize": (2 ** 27 - 1, [op("partials", "in", 128, True), op("row_ab", "out", 8, True, narrow=True)],
                          "tests/test_gpu_fused_epilogues.py test_ln_stats_finalize_every_row_kind: FC.ab_bounds"),
    "linear_smallk_f32": (ROWS, [op("x", "in", 8, True, narrow=True), op("y", "out", _F, True)],
                          "tests/test_gpu_iqm.py test_residual_layernorm_combine_smallk_dropcls: 1e-6 + 1e-6 |ref|"),
    "linear_smallk_f16": (ROWS, [op("x", "in", 8, True, narrow=True), op("y", "out", _H, False)],
                          "tests/test_gpu_iqm.py test_residual_layernorm_combine_smallk_dropcls: 2e-3 + 2e-3 |ref|"),
    # H = 16 heads of 64: one q row expands to 16 rows of 1024, 64 KiB; rows * H = 2^20 + 592 < 2^31
    "head_expand": (HEAD_ROWS, [op("q", "in", _F, True, narrow=True), op("qm", "out", HEAD_H * _F, True)],
                    "tests/test_gpu_iqm.py test_cross_rows_equals_projected_cross_attention: allclose at 1e-7 (+ 1e-5 |ref|)"),
    "head_diag": (HEAD_ROWS, [op("full", "in", HEAD_H * _F, True), op("ctx", "out", _F, True, narrow=True)],
                  "a copy of the diagonal blocks: equality"),
    # the largest grids that remain allowed: 2^24 - 1 workgroups
    "head_expand_max": (HEAD_MAX_ROWS, [op("q", "in", 4 * HEAD_MAX_D, True), op("qm", "out", 3 * 4 * HEAD_MAX_D, True)],
                        "as head_expand"),
    "head_diag_max": (GRID_MAX - 1, [op("full", "in", 2 * 4 * 128, True), op("ctx", "out", 4 * 128, True)], "as head_diag"),
    "layernorm_max": (ROWS4_MAX, [op("x", "in", 4 * 256, True), op("out", "out", 2 * 256, False)],
                      "tests/test_gpu_parity.py test_layernorm: 2e-3 + 1e-2 |ref|"),
    "bias_grad": (ROWS, [op("dz", "in", _F, True)], "small integers: equality (test_wgrad_exact_integers' rule)"),
    "layernorm_param_grad": (ROWS, [op("x", "in", _F, True), op("d_y", "in", _F, True)],
                             "d_b: integers, equality; d_w: the summation bound of BB.wgrad_bound for this row count"),
}
LN_TOL = {"layernorm_f32": (2e-6, 1e-5), "layernorm_f16": (2e-3, 1e-2), "layernorm_bf16": (2e-2, 1e-2)}
SPLIT_LN_TOL = (6e-6, 2.0 ** -14)
MIX_WEIGHT = 0.1
LN_EPS = 1e-5
IQB_MAX_CHUNKS = 64                        # csrc/kernels.h IQB_MAX_CHUNKS: partial sums that a second pass adds


@functools.lru_cache(maxsize=None)
def ln_base():
    """x [P, 1024], gamma, beta and the fp64 LayerNorm of tests/test_gpu_parity.py test_layernorm's draw"""
    x = rnd("ln.x", (P, WIDTH), 3.0, 0.7)
    w, b = rnd("ln.w", (WIDTH,), 0.2, 1.0), rnd("ln.b", (WIDTH,), 0.2)
    ref = torch.nn.functional.layer_norm(x.double(), (WIDTH,), w.double(), b.double(), LN_EPS)
    return x, w, b, ref


@functools.lru_cache(maxsize=None)
def mix_base():
    """x, a [P, 1024] of test_adapter_mix's draw and the fp64 mix"""
    x, a = rnd("mix.x", (P, WIDTH), 2.0), rnd("mix.a", (P, WIDTH), 0.3)
    xd, ad = x.double(), a.double()
    ref = MIX_WEIGHT * (ad * xd.norm(dim=-1, keepdim=True) / ad.norm(dim=-1, keepdim=True)) + (1 - MIX_WEIGHT) * xd
    return x, a, ref


@functools.lru_cache(maxsize=None)
def combine_base():
    a, b, c = rnd("c3.a", (P, WIDTH), 2.0, 0.5), rnd("c3.b", (P, WIDTH)), rnd("c3.c", (P, WIDTH))
    w, bias = rnd("c3.w", (WIDTH,), 0.2, 1.0), rnd("c3.bias", (WIDTH,), 0.2)
    ln = torch.nn.functional.layer_norm((a + b).double(), (WIDTH,), w.double(), bias.double(), 1e-12)
    return a, b, c, w, bias, ln, 0.4 * a.double() + 0.3 * b.double() + 0.3 * c.double()


@functools.lru_cache(maxsize=None)
def ln_backward_base():
    """BB's "plain" kind at P rows -> (x, gamma, dy, d_resid), fp64 autograd dx + d_resid, fp64 terms"""
    x, w = rnd("lnb.x", (P, WIDTH), 2.0) + 0.3, rnd("lnb.w", (WIDTH,), 0.1) + 1.0
    dy, dr = rnd("lnb.dy", (P, WIDTH)), rnd("lnb.dr", (P, WIDTH))
    x64 = x.double().requires_grad_(True)
    torch.nn.functional.layer_norm(x64, (WIDTH,), w.double(), None, BB.LN_EPS).backward(dy.double())
    _, terms = BB.ln_backward_formula(x.double(), w.double(), dy.double())
    return (x, w, dy, dr), x64.grad + dr.double(), terms + dr.double().abs()


@functools.lru_cache(maxsize=None)
def mix_backward_base():
    """BB's "plain" kind at P rows -> (u, z, dy), fp64 autograd (dz, du), fp64 terms (dz, du)"""
    u, z, dy = rnd("mixb.u", (P, WIDTH), 1.5), rnd("mixb.z", (P, WIDTH)), rnd("mixb.dy", (P, WIDTH))
    u64, z64 = u.double().requires_grad_(True), z.double().requires_grad_(True)
    a = torch.nn.functional.leaky_relu(z64, BB.SLOPE)
    y = MIX_WEIGHT * a * u64.norm(dim=-1, keepdim=True) / a.norm(dim=-1, keepdim=True) + (1 - MIX_WEIGHT) * u64
    y.backward(dy.double())
    _, _, t_dz, t_du = BB.mix_backward_formula(u.double(), z.double(), dy.double(), MIX_WEIGHT)
    return (u, z, dy), (z64.grad, u64.grad), (t_dz, t_du)


@functools.lru_cache(maxsize=None)
def act_base(act):
    """zy, d_y [P, 1024] (tests/iqm_query_backward_cases.py act_inputs' draw: 0 and +-10 among the values; the ReLU's zy
    is the activation's output) and the fp64 d_z"""
    z = rnd(f"act.{act}.z", (P, WIDTH), 1.5)
    z[:, 3], z[:, 4], z[:, 5], z[:, WIDTH - 1] = 0.0, 10.0, -10.0, 0.0
    g = rnd(f"act.{act}.dy", (P, WIDTH))
    if act == 2:
        z = torch.relu(z)
        return z, g, torch.where(z.double() > 0, g.double(), torch.zeros((), dtype=torch.float64))
    z64 = z.double().requires_grad_(True)
    torch.nn.functional.gelu(z64).backward(g.double())
    return z, g, z64.grad


@functools.lru_cache(maxsize=None)
def smallk_base():
    """x [P, 2], W [1024, 2], bias [1024] (test_residual_layernorm_combine_smallk_dropcls' draws) and the fp64 y"""
    x, W, bias = rnd("sk.x", (P, 2), 0.05), rnd("sk.W", (WIDTH, 2)), rnd("sk.bias", (WIDTH,), 0.1)
    return x, W, bias, x.double() @ W.double().t() + bias.double()


@functools.lru_cache(maxsize=None)
def head_base(D=WIDTH, H=HEAD_H):
    """q [P, D]; the expanded rows [P, H * D] = q * hd^-1/2 inside head h's hd columns of row (r, h), zero outside; and
    `full` [P, H * D] with its diagonal blocks [P, D]"""
    q = rnd(f"he.q.{D}.{H}", (P, D))
    hd = D // H
    want = torch.zeros(P, H, D, dtype=torch.float64)
    for h in range(H):
        want[:, h, h * hd:(h + 1) * hd] = q[:, h * hd:(h + 1) * hd].double() * float(torch.tensor(hd ** -0.5, dtype=torch.float32))
    full = rnd(f"he.full.{D}.{H}", (P, H, D))
    diag = torch.cat([full[:, h, h * hd:(h + 1) * hd] for h in range(H)], dim=1)
    return q, want.view(P, -1), full.view(P, -1).contiguous(), diag.contiguous()


# aaclip_drop_cls_rows takes int arguments: B images of L rows, fp32 rows of 1024.  L - 1 = 1024 rows of every image go
# to rows [2, 1026) of 1027; source 4 GiB + 14.6 MiB, destination 4 GiB + 22.6 MiB.  L is no multiple of P, so the CLS
# rows fall on every phase.
DROP_CLS = dict(B=1027, L=1025, E=WIDTH, rows_per_image=1027, row_off=2)
DROP_CLS_CASE = (DROP_CLS["B"] * DROP_CLS["L"], [op("src", "in", _F, True)],
                 DROP_CLS["B"] * DROP_CLS["rows_per_image"], [op("dst", "out", _F, True)])


def drop_cls_source(rho, B, L, E, rows_per_image, row_off):
    """destination rows rho (numpy or torch integers) -> (written, source row): row (b, row_off + t) <- row (b, 1 + t)"""
    b, t = rho // rows_per_image, rho % rows_per_image
    written = (t >= row_off) & (t < row_off + L - 1)
    return written, b * L + 1 + (t - row_off)


def reduction_bound(rows, mag, partials):
    """BB.wgrad_bound's rule for `rows` terms whose partial sums a second pass adds: (rows + partials) 2^-24 sum |terms|"""
    return (rows + partials) * BB.EPS24 * mag


def wrapped_counts(rows, wrap_rows, period=P):
    """counts() of a kernel whose row offset wraps after wrap_rows rows: row r >= wrap_rows reads row r - wrap_rows"""
    return counts(min(rows, wrap_rows), period) + counts(max(rows - wrap_rows, 0), period)


# The summation bound of a reduction over 10^6 rows is (rows + 64) 2^-24 sum |terms|, 6 % of the sum of magnitudes: it
# cannot see a wrapped row offset, which moves 2051 of the rows -- and only 9 of them onto another phase.  The sums that
# can be made exact are therefore made exact: small integers, every partial sum below 2^24 in any order, equality.
@functools.lru_cache(maxsize=None)
def bias_grad_base(rows=ROWS, wrap_rows=None):
    """dz [P, 1024] of integers in [-3, 7], asymmetric in both dimensions; the exact sum_j count_j dz_j (fp64) -- with
    wrap_rows: what a row offset that wraps there would give"""
    g = torch.Generator().manual_seed(1000 * P + 7)
    dz = torch.randint(-3, 4, (P, WIDTH), generator=g).float()
    dz += (torch.arange(P).float() % 5)[:, None] * (torch.arange(WIDTH) % 3 == 0).float()[None, :]
    assert float(dz.abs().max()) <= 7 and rows * 7 < 2 ** 24
    c = counts(rows) if wrap_rows is None else wrapped_counts(rows, wrap_rows)
    return dz, (torch.from_numpy(c).double()[:, None] * dz.double()).sum(0)


@functools.lru_cache(maxsize=None)
def ln_param_grad_base(rows=ROWS, wrap_rows=None):
    """x, d_y [P, 1024] -> fp64 (d_w, d_b) = sum_j count_j (dy_j xhat_j, dy_j) and the sum of |dy xhat|.  d_y is
    sign(xhat) * (1 + j % 7) in row j: integers, so d_b is exact and compared for equality; the terms of d_w all have one
    sign, so a share of the rows that is left out shows against the bound."""
    x = rnd("lpg.x", (P, WIDTH), 2.0) + 0.3
    xd = x.double()
    xc = xd - xd.mean(-1, keepdim=True)
    xh = xc * torch.rsqrt((xc * xc).mean(-1, keepdim=True) + LN_EPS)
    dy = (torch.sign(xh) * (1 + torch.arange(P) % 7)[:, None]).float()
    assert float(dy.abs().max()) <= 7 and rows * 7 < 2 ** 24 and bool((dy != 0).all())
    c = torch.from_numpy(counts(rows) if wrap_rows is None else wrapped_counts(rows, wrap_rows)).double()[:, None]
    t = dy.double() * xh
    assert bool((t >= 0).all())
    return x, dy, ((c * t).sum(0), (c * dy.double()).sum(0)), (c * t.abs()).sum(0)


# ------------------------------------------------------------------------------------------------ group 2: products
GEMM_N, GEMM_K, GEMM_LD = 256, 128, 16384          # ld in elements of the operand's type (halves for split rows)
GEMM_M16 = 2 ** 17 + 301                           # 16-bit and split A: 32 KiB per row, 4 GiB + 9.4 MiB
GEMM_M32 = 2 ** 16 + 301                           # fp32 A: 64 KiB per row
GEMM_ET = {F32: 1e-5, F16: 1.5e-3, BF16: 1.2e-2}   # tests/test_gpu_parity.py test_gemm_epilogues: output rounding
GEMM_F32_OUT_TOL = (2e-5, 1e-5)                    # the same test's resid and leaky epilogues
GEMM_SPLIT_TOL = (3e-4, 1e-4)                      # tests/test_gpu_split.py test_gemm_split_epilogues
GEMM_EPIS = (EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESID, EPI_ACT_F32)
GEMM_VARIANTS = (0, 1)                             # the automatic 256-row tiles; always the 128 x 128 tile


def gemm_rows(code):
    return GEMM_M32 if code == F32 else GEMM_M16


def gemm_operands(code, epi):
    """the scaling operands of one aaclip_gemm case at lda = ldc = GEMM_LD"""
    a_es = 4 if code == F32 else 2
    if epi in (EPI_BIAS_RESID, EPI_ACT_F32):
        o_es, o32 = 4, True
    else:
        o_es, o32 = (4, True) if code == F32 else (2, False)
    return [op("A", "in", GEMM_LD * a_es, code == F32), op("out", "inout" if epi == EPI_BIAS_RESID else "out",
                                                          GEMM_LD * o_es, o32)]


GEMM_CASES = {(code, epi): (gemm_rows(code), gemm_operands(code, epi)) for code in (F32, F16, BF16, F16X2)
              for epi in GEMM_EPIS}


@functools.lru_cache(maxsize=None)
def gemm_base():
    """A [P, K], W [N, K], bias [N], residual rows [P, N] (test_gemm_epilogues' draws)"""
    return (rnd("g.a", (P, GEMM_K)), rnd("g.w", (GEMM_N, GEMM_K), GEMM_K ** -0.5), rnd("g.b", (GEMM_N,), 0.5),
            rnd("g.x", (P, GEMM_N), 2.0))


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def gemm_reference(A_seen, W_seen, bias, resid, epi):
    """fp64 of one epilogue on the operand values the kernel sees (already rounded to its type); EPI_ACT_F32 runs with
    LeakyReLU and no bias, EPI_BIAS with the first 64 columns scaled by 1/8, as the existing tests call them"""
    acc = A_seen.double() @ W_seen.double().t()
    if epi == EPI_BIAS:
        ref = acc + bias.double()
        ref[:, :64] *= 0.125
        return ref
    if epi == EPI_BIAS_GELU:
        return gelu64(acc + bias.double())
    if epi == EPI_BIAS_RESID:
        return resid.double() + acc + bias.double()
    return torch.where(acc > 0, acc, 0.01 * acc)


WGRAD_O = WGRAD_I = 256
WGRAD_LD = 16384
WGRAD_ROWS = 2 ** 16 + 301                         # fp32 rows of 64 KiB: both operands 4 GiB + 18.8 MiB
WGRAD_CASE = (WGRAD_ROWS, [op("dz", "in", 4 * WGRAD_LD, True), op("u", "in", 4 * WGRAD_LD, True)])


@functools.lru_cache(maxsize=None)
def wgrad_base(rows=WGRAD_ROWS):
    """Small integers as BB.wgrad_exact_case draws them, P rows: |dz| <= 13, |u| <= 6, so every partial sum is below
    rows * 78 < 2^24 and any summation order is exact in fp32 -> (dz, u, exact dw of the periodic operands)"""
    g = torch.Generator().manual_seed(1000 * P + WGRAD_O + WGRAD_I)
    dz = torch.randint(-3, 4, (P, WGRAD_O), generator=g).float()
    u = torch.randint(-2, 3, (P, WGRAD_I), generator=g).float()
    dz += (torch.arange(P).float() % 5)[:, None] * (torch.arange(WGRAD_O) % 3 == 0).float()[None, :]
    dz[0] += torch.arange(WGRAD_O).float() % 7
    u += (torch.arange(P).float() % 3)[:, None] * (torch.arange(WGRAD_I) % 5 == 1).float()[None, :]
    u[-1] += torch.arange(WGRAD_I).float() % 3
    assert float(dz.abs().max()) <= 13 and float(u.abs().max()) <= 6 and rows * 78 < 2 ** 24
    c = torch.from_numpy(counts(rows)).double()[:, None]
    return dz, u, (c * dz.double()).t() @ u.double()


# aaclip_gemm_fused at the same extents (M = GEMM_M16, strides GEMM_LD, the 256-row-tile kernels), one case per form.
# out16, stats_out and row_ab have no stride argument: they are contiguous rows of 512, 32 and 8 bytes (`narrow`).
_L16 = GEMM_LD * 2
FUSED_CASES = {
    # residual epilogue reading `resid` at the stride of out, writing the 16-bit rows and their slice statistics
    "out16_stats": (GEMM_M16, [op("A", "in", _L16, False), op("resid", "in", 2 * _L16, True), op("out", "out", 2 * _L16, True),
                               op("out16", "out", 2 * GEMM_N, False, narrow=True),
                               op("stats_out", "out", GEMM_N // 64 * 8, True, narrow=True)]),
    # LayerNorm folded into a GELU product: (rstd, -mean rstd) per row, column sums of the folded weight
    "row_ab_col_s": (GEMM_M16, [op("A", "in", _L16, False), op("row_ab", "in", 8, True, narrow=True),
                                op("out", "out", _L16, False)]),
    # split product whose bias epilogue writes the attention kernel's e4m3 records
    "out_qk8": (GEMM_M16, [op("A", "in", _L16, False), op("out", "out", _L16, False)]),
}
FUSED_QK8 = 128                                    # out_qk8: record columns of the N = 256 outputs


@functools.lru_cache(maxsize=None)
def fused_fold_base():
    """tests/test_gpu_fused_epilogues.py test_folded_chain_against_fp64_and_the_layernorm_route at D = K = 128, N = 256,
    'plain' rows: fp16 rows x16 [P, 128], their (rstd, b) pairs (FC.finalize_emulated), the folded weight, its column
    sums and bias, and fp64 gelu(LN(x16) W^T + bias)"""
    import fused_epilogue_cases as FC
    D = GEMM_K
    W, bias, gamma, beta = FC.chain_params(D, GEMM_N)
    x16 = FC.round16(FC.rows("plain", P, D), "fp16")
    ab = FC.finalize_emulated(FC.slice_stats_emulated(x16), D)
    wf, col_s, fb = FC.fold_weights(W, bias, gamma, beta, "fp16")
    return x16.half(), ab, wf, col_s, fb, FC.chain_reference64(x16, W, bias, gamma, beta, True)


@functools.lru_cache(maxsize=None)
def fused_qk8_base():
    """tests/test_gpu_fused_epilogues.py test_out_qk8_records_byte_for_byte's construction at P rows: A in {0, 1} (three
    per row), W in {0, 1, 2^-13}, integer bias, the first 64 columns halved -- every output is exactly hi + lo8 * 2^-10,
    so every byte of the row is the host builder's -> (A, W, bias, the record rows [P, 2 N + 2 out_qk8] bytes)"""
    import fused_epilogue_cases as FC
    N, K, Q = GEMM_N, GEMM_K, FUSED_QK8
    g = torch.Generator().manual_seed(11)
    W = torch.tensor([0.0, 1.0, 2.0 ** -13])[torch.randint(0, 3, (N, K), generator=g)]
    bias = torch.randint(0, 3, (N,), generator=g).float()
    m = torch.arange(P)
    A = torch.zeros(P, K)
    for mul, add in ((1, 0), (7, 3), (13, 5)):
        A[m, (mul * m + add) % K] = 1.0
    ref = A.double() @ W.double().t() + bias.double()
    ref[:, :64] *= 0.5
    val = ref.float()
    assert torch.equal(val.double(), ref)
    return A, W, bias, FC.qk8_records_cols(val, Q)


# ------------------------------------------------------------------------------------------------ group 3: attention
# The packed q|k|v rows are [B * L, planes of H heads]: the extent is reached through the HEAD count, so the period runs
# over heads -- head h of image b holds base[(b * H + h) % period], an [L, 192] slice -- and the reference is `period`
# heads of an L-token attention.  Short rows: (L, H) = (42, 65535), an image's fp32 rows 2 113 896 960 bytes, 33.6 MB
# below 2^31, so image 1 holds the 2^31 crossing; B = 2 as stated, and B = 3 so that the fp32 and split operands pass
# 2^32 as well (16-bit: 2^31).  Long rows (the other kernel family): L = 513, H = 5450 -- one more head is refused.
ATTN_SHORT = (42, 65535, P)                        # L, H, period
ATTN_LONG = (513, 5450, 127)
ATTN_QK8_PERIOD = 3                                # the record form: the three images of the existing record test's case
ATTN_BATCHES = (2, 3)
ATTN_TOL = {"f32": (2e-5, 1e-5), "f16": (3e-3, 1e-2), "bf16": (2.5e-2, 3e-2),      # tests/test_gpu_parity.py test_attention
            "split16": (4e-4, 1e-3), "qk8": (4e-4, 1e-3)}     # test_attention_split, test_qk8_attention_on_host_built_records
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453


@functools.lru_cache(maxsize=None)
def attention_heads(L, period, log2q):
    """fp32 [period * L, 192]: q|k|v of `period` single heads, q scaled as the existing tests scale it (0.6, times log2 e
    for the entries that take q in log2 units)"""
    qkv = rnd(f"attn.{L}.{period}", (period * L, 192))
    qkv[:, :64] *= 0.6 * (LOG2E if log2q else 1.0)
    return qkv


def attention_reference(seen, L, period, log2q):
    """fp64 softmax(q k^T) v per head of the values the kernel sees -> [period, L, 64]"""
    f = seen.double().view(period, L, 3, 64)
    q, k, v = f[:, :, 0] * (LN2 if log2q else 1.0), f[:, :, 1], f[:, :, 2]
    return torch.softmax(q @ k.transpose(-1, -2), -1) @ v


def attention_row_bytes(form, H):
    """bytes of one packed q|k|v row and of one context row"""
    return {"f32": (768 * H, 256 * H), "f16": (384 * H, 128 * H), "bf16": (384 * H, 128 * H),
            "split16": (768 * H, 256 * H), "qk8": (640 * H, 256 * H)}[form]


def attention_phase_at(offset, B, L, H, period, plane_bytes=256, row_bytes=None):
    """the phase of the head that holds byte `offset` of fp32 packed rows (split16: plane_bytes = 128; the e4m3 records:
    plane_bytes = 128 and row_bytes = 640 H)"""
    return attention_slot_at(offset, B, L, H, period, plane_bytes, row_bytes)[0]


def attention_slot_at(offset, B, L, H, period, plane_bytes=256, row_bytes=None):
    """where in the base byte `offset` of the packed rows comes from: (phase of its head, token row, plane, byte within
    the head's slice) -- two offsets hold the same base byte only if all four agree"""
    row_bytes = row_bytes or 768 * H
    row, col = divmod(offset, row_bytes)
    return (((row // L) * H + (col % (H * plane_bytes)) // plane_bytes) % period, row % L, col // (H * plane_bytes),
            col % plane_bytes)


# ------------------------------------------------------------------------------------------------ group 4: metrics
MP = 65537                                         # distinct score values; the labels' period is 3 MP
METRIC_SIZES = (2 ** 29 + 3, 2 ** 31 - 1)
# scores per image of the range entry: 2^29 + 3 = 5 * 7 * 1901 * 8069 in images of 35 is 15 339 169 images, the most that
# stay below the 2^24 segments one call takes; 2^31 - 1 is prime: no image size divides it
METRIC_PER_IMAGE = {2 ** 29 + 3: 35, 2 ** 31 - 1: 0}
METRIC_KINDS = ("plain", "passthrough")
METRIC_CASES = {(n, kind): (n, [op("scores", "in", 4, True)]) for n in METRIC_SIZES for kind in METRIC_KINDS}


@functools.lru_cache(maxsize=None)
def metric_base(kind):
    """-> (s float32 [MP] with MP distinct bit patterns, l uint8 [3 MP]).  'plain': normal scores, normalised by the code
    under test; 'passthrough': max == 1 exactly, negatives, -0.0 and +0.0 (two bit patterns, one key): taken as they are"""
    rng = np.random.default_rng(65537 + len(kind))
    if kind == "plain":
        s = np.unique(rng.normal(size=2 * MP).astype(np.float32))
        s = s[s != 0]
    else:
        assert kind == "passthrough"
        s = np.unique(rng.uniform(-0.999, 0.999, size=2 * MP).astype(np.float32))
        s = s[s != 0]
    s = s[rng.permutation(s.size)[:MP]]
    if kind == "passthrough":
        s[:3] = np.array([1.0, -0.0, 0.0], np.float32)
        assert s.max() == 1 and s.min() < 0
    assert s.size == MP and np.unique(s.view(np.uint32)).size == MP
    l = (rng.random(3 * MP) < 0.3).astype(np.uint8)
    l[0], l[1] = 1, 0
    return np.ascontiguousarray(s, np.float32), l


def pair_counts(n, labels3):
    """-> (pos, neg) int64 [MP]: how often value j occurs with a positive / a negative label among i < n, for scores
    s[i % MP] and labels l[i % (3 MP)]: i % MP == j means i % (3 MP) is one of j, j + MP, j + 2 MP"""
    c = counts(n, 3 * MP).reshape(3, MP)
    lab = (np.asarray(labels3).reshape(3, MP) != 0)
    return (c * lab).sum(0), (c * ~lab).sum(0)


def expand(n, s, labels3):
    i = np.arange(n)
    return s[i % MP], labels3[i % (3 * MP)]


def curve_metrics_weighted(values, pos, neg):
    """AUROC, AP, F1-max and its threshold of float32 `values` that occur pos[j] times with a positive and neg[j] times
    with a negative label: metrics_device_cases.curve_sums on a weighted histogram, in exact Python / int64 integers and
    fp64 (values with one key -- -0.0 and +0.0 -- are one group).  F1-max: the largest 2 tp / (2 tp + fp + fn) as a
    fraction, the higher threshold among equal ones (tests/f1max_cases.py brute_force)."""
    values = np.asarray(values, np.float32)
    pos, neg = np.asarray(pos, np.int64), np.asarray(neg, np.int64)
    keys = MD.make_keys(values, np.zeros(values.size, np.uint8), False)
    uk, inv = np.unique(keys, return_inverse=True)
    gp, gn = np.zeros(uk.size, np.int64), np.zeros(uk.size, np.int64)
    np.add.at(gp, inv, pos)
    np.add.at(gn, inv, neg)
    live = (gp + gn) > 0
    uk, gp, gn = uk[live], gp[live], gn[live]
    rep = {}
    for k, v in zip(keys.tolist(), values.tolist()):
        rep.setdefault(k, v + 0.0)                               # -0.0 and +0.0: the threshold is reported as +0.0
    gv = np.array([rep[int(k)] for k in uk], np.float32)
    Ptot, Ntot = int(gp.sum()), int(gn.sum())
    tp = np.cumsum(gp[::-1])[::-1]                               # counts down to and including a group, from the top
    fp = np.cumsum(gn[::-1])[::-1]
    tp0, fp0 = np.concatenate([tp[1:], [0]]), np.concatenate([fp[1:], [0]])
    num = sum(int(a) * int(b) for a, b in zip(fp - fp0, tp + tp0))
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = ((tp - tp0).astype(np.float64) / np.float64(Ptot)) * (tp.astype(np.float64) / (tp + fp).astype(np.float64))
    ap = float(np.sum(terms[::-1]))
    best = None
    for g in range(uk.size):                                     # ascending: a later equal F1 has the higher threshold
        t, f = int(tp[g]), int(fp[g])
        a, b = 2 * t, 2 * t + f + (Ptot - t)
        if best is None or a * best[1] >= best[0] * b:
            best = (a, b, g)
    g = best[2]
    return {"num": num, "P": Ptot, "N": Ntot, "groups": int(uk.size), "ap": ap, "auroc": num / (2 * Ptot * Ntot),
            "tp": int(tp[g]), "fp": int(fp[g]), "fn": Ptot - int(tp[g]), "threshold": float(gv[g]),
            "f1": best[0] / best[1], "start": int((gp + gn)[:g].sum()), "keys": uk, "group_pos": gp, "group_neg": gn,
            "group_values": gv}


# ------------------------------------------------------------------------------------------------ group 5: refusals
# A message of csrc/capi.hip states a size limit when it holds one of these
LIMIT_WORDS = ("2^31", "2^27", "2 GiB", "too many rows", "too many workgroups", "grid limit", "32-bit row offsets")
N31 = 1 << 31
BIG = 1 << 40                                      # a workspace size that no check finds too small


def limit_messages(path=CAPI):
    """every string literal of csrc/capi.hip that states a size limit"""
    src = open(path).read()
    found = [m.group(1) for m in re.finditer(r'"((?:[^"\\]|\\.)*)"', src)]
    return sorted({s for s in found if any(w in s for w in LIMIT_WORDS)})


# (id, entry, arguments, the literal of capi.hip that the call must meet, prefix the message must carry).
# Arguments: "i<k>" an input pointer, "o<k>" a poisoned output, "w" the workspace, "xs" / "dxs" a host array of one
# segment pointer, "bw" a zeroed aaclip_block_weights, "plan31" a bootstrap plan of n = 2^31, "optim" a tensor list with
# one tensor of one element too many; numbers as they are.
# Every call is the smallest step past its limit with everything else valid, so that the limit is what refuses it.
_AT = "L * 3 * 64 * H * 4 must stay below 2^31 (32-bit row offsets)"
_R4 =": too many rows (one workgroup per 4 rows, below 2^24 workgroups: rows <= 2^26 - 4)"
REFUSALS = [
    ("attention.B", "aaclip_attention", [F16, "i0", "o0", 65536, 1, 1, 0, None], "attention: grid limit", ""),
    ("attention.H", "aaclip_attention", [F16, "i0", "o0", 1, 1, 65536, 0, None], "attention: grid limit", ""),
    ("attention.span", "aaclip_attention", [F32, "i0", "o0", 1, 43, 65535, 0, None], "attention: " + _AT, ""),
    ("attention_log2q.span", "aaclip_attention_log2q", [F16, "i0", "o0", 2, 43, 65535, 0, None], "attention: " + _AT, ""),
    ("attention.workgroups", "aaclip_attention", [F16, "i0", "o0", 16385, 1, 65535, 0, None],
     "attention: too many workgroups", ""),
    ("attention_split.B", "aaclip_attention_split", ["i0", "o0", 65536, 1, 1, 0, 0, 0, 1, None],
     "attention_split: grid limit", ""),
    ("attention_split.span", "aaclip_attention_split", ["i0", "o0", 1, 43, 65535, 0, 0, 0, 1, None],
     "attention_split: " + _AT, ""),
    ("attention_split.span_long", "aaclip_attention_split", ["i0", "o0", 2, 513, 5451, 0, 1, 1, 1, None],
     "attention_split: " + _AT, ""),
    ("attention_split.workgroups", "aaclip_attention_split", ["i0", "o0", 16385, 1, 65535, 0, 0, 0, 1, None],
     "attention_split: too many workgroups", ""),
    ("ln_stats_finalize.rows", "aaclip_ln_stats_finalize", ["i0", "o0", 1 << 27, 256, 1e-5, None],
     "ln_stats_finalize: rows must be in 1 .. 2^27 - 1", ""),
    ("cross_rows_backward.B", "aaclip_cross_rows_backward",
     [F16, "i0", "i1", "i2", "o0", "o1", 0, 0, 65536, 16, 100, 768, "w", BIG, None],
     "cross_rows_backward: grid limit (B <= 65535)", ""),
    ("cross_rows_levels.span", "aaclip_cross_rows_levels",
     [F16, "i0", "xs", 1, "o0", 1, 16, 1024, 0, 10, 768, 1 << 20, "w", BIG, None],
     "cross_rows_levels: an image's rows must span < 2 GiB", ""),
    ("cross_rows_levels_backward.span", "aaclip_cross_rows_levels_backward",
     [F16, "i0", "xs", 1, "i2", "o0", "dxs", 0, 1, 16, 1024, 0, 10, 768, 1 << 20, "w", BIG, None],
     "cross_rows_levels_backward: an image's rows must span < 2 GiB", ""),
    ("head_expand.rows", "aaclip_head_expand", [F32, "i0", "o0", 1 << 20, 16, 1024, 0.125, None],
     "head_expand: too many rows (one workgroup per expanded row: rows * H < 2^24)", ""),
    ("head_diag.rows", "aaclip_head_diag", ["i0", "o0", 1 << 24, 1, 64, None],
     "head_diag: too many rows (one workgroup per row: rows < 2^24)", ""),
    ("split3_rows.rows", "aaclip_split3_rows", ["i0", "o0", (1 << 29) - 31, 64, None],
     "split3_rows: too many rows (one thread per 8 elements, below 2^24 workgroups: rows * K <= 2^35 - 2048)", ""),
    ("layernorm.rows", "aaclip_layernorm", ["i0", "i1", "i2", "o0", F16, ROWS4_REFUSED, 256, 1e-5, None], _R4, "layernorm"),
    ("layernorm_split.rows", "aaclip_layernorm_split", ["i0", "i1", "i2", "o0", ROWS4_REFUSED, 256, 1e-5, 1, None],
     _R4, "layernorm_split"),
    ("adapter_mix.rows", "aaclip_adapter_mix", ["o0", "i0", ROWS4_REFUSED, 256, 0.1, None], _R4, "adapter_mix"),
    ("adapter_mix_fold.rows", "aaclip_adapter_mix_fold", [F16, "o0", "i0", ROWS4_REFUSED, 256, 0.1, "o1", "o2", None],
     _R4, "adapter_mix_fold"),
    ("residual_layernorm.rows", "aaclip_residual_layernorm", ["i0", "i1", "i2", "i3", "o0", ROWS4_REFUSED, 256, 1e-5, None],
     _R4, "residual_layernorm"),
    ("layernorm_backward.rows", "aaclip_layernorm_backward", ["i0", "i1", "i2", "i3", "o0", ROWS4_REFUSED, 256, 1e-5, None],
     _R4, "layernorm_backward"),
    ("adapter_mix_backward.rows", "aaclip_adapter_mix_backward", ["i0", "i1", "i2", "o0", "o1", ROWS4_REFUSED, 256, 0.1, None],
     _R4, "adapter_mix_backward"),
    ("metrics_range.images", "aaclip_metrics_range", ["i0", "i1", 1 << 25, 2, "o1", "o0", "w", BIG, None],
     "metrics_range: too many workgroups (one or more per image: n / per_image must stay below 2^24)", ""),
    ("metrics_threshold.images", "aaclip_metrics_threshold",
     ["i0", "i1", 1 << 25, 2, "i2", "i3", "o0", None, "o1", "w", BIG, None],
     "metrics_threshold: too many workgroups (one or more per image: n / per_image must stay below 2^24)", ""),
    ("small_attention_backward.B", "aaclip_small_attention_backward",
     ["i0", "i1", "i2", "i3", "o0", "o1", "o2", 65536, 2, 10, 8, 96, 0.1, None],
     "small_attention_backward: grid limit (B, H <= 65535)", ""),
    ("layernorm_param_grad.rows", "aaclip_layernorm_param_grad",
     ["i0", "i1", "o0", "o1", ROWS4_REFUSED, 64, 1e-5, "w", BIG, None], _R4, "layernorm_param_grad"),
    ("blocks.span", "aaclip_blocks", ["o0", "bw", 1, 0.1, 1, 699051, 256, 4, 1024, 0, F16, "w", BIG, None],
     "block: sequence too long for the attention kernel's 32-bit row offsets", ""),
    ("blocks.rows", "aaclip_blocks", ["o0", "bw", 1, 0.1, 8192, 8192, 256, 4, 1024, 0, F16, "w", BIG, None],
     "block: too many rows", ""),
    ("gemm_wgrad.rows", "aaclip_gemm_wgrad", ["i0", 256, "i1", 256, "o0", N31, 256, 256, "w", BIG, None],
     "gemm_wgrad: rows must be positive (and below 2^31)", ""),
    ("block_backward_long.rows", "aaclip_block_backward_long",
     ["i0", "bw", "bw", 0.1, 8192, 8192, 256, 4, 1024, 0, "i1", "o0", "o1", "w", BIG, None],
     "too many rows", "block_backward: "),
    ("tap_head_backward.rows", "aaclip_tap_head_backward",
     ["i0", "i1", "i2", "i3", "i4", 0, "i5", None, None, None, "o0", "o1", None, 8192, 8192, 256, 256, "w", BIG, None],
     "tap_head_backward: too many rows", ""),
    ("metrics_range.n", "aaclip_metrics_range", ["i0", "i1", N31, 0, None, "o0", "w", BIG, None],
     "metrics_range: n must be 2 .. 2^31 - 1", ""),
    ("metrics_normalise.n", "aaclip_metrics_normalise", ["i0", "o0", N31, "i1", None],
     "metrics_normalise: n must be 1 .. 2^31 - 1", ""),
    ("metrics_sort.n", "aaclip_metrics_sort", ["i0", "i1", N31, 0, "o0", "o1", "o2", "w", BIG, None],
     "metrics_sort: n must be 2 .. 2^31 - 1", ""),
    ("metrics_curve.n", "aaclip_metrics_curve", ["i0", "i1", N31, 0, "o0", "w", BIG, None],
     "metrics_curve: n must be 2 .. 2^31 - 1", ""),
    ("bootstrap_curves.n", "aaclip_bootstrap_curves", ["plan31", "i0", "i1", "i2", "o0", "w", BIG],
     "bootstrap_curves: n must be 1 .. 2^31 - 1", ""),
    ("optim_grad_norm.n", "aaclip_optim_grad_norm", ["optim", 1.0, "o0", "w", BIG, None],
     "a tensor has more than 2^27 * 16384 elements", "optim_grad_norm: "),
    ("metrics_f1max.n", "aaclip_metrics_f1max", ["i0", "i1", N31, 0, "o0", "w", BIG, None],
     "metrics_f1max: n must be 2 .. 2^31 - 1", ""),
    ("metrics_threshold.n", "aaclip_metrics_threshold",
     ["i0", "i1", N31, 0, "i2", "i3", "o0", None, "o1", "w", BIG, None], "metrics_threshold: n must be 2 .. 2^31 - 1", ""),
    ("metrics_regions.n", "aaclip_metrics_regions", ["i0", 2, 32768, 32768, 8, "o0", "o1", "o2", "w", BIG, None],
     "metrics_regions: images, H, W must be positive with 2 .. 2^31 - 1 pixels in all", ""),
    ("metrics_sort_pairs.n", "aaclip_metrics_sort_pairs", ["i0", "i1", N31, "o0", "o1", "w", BIG, None],
     "metrics_sort_pairs: n must be 2 .. 2^31 - 1", ""),
    ("metrics_pro_curve.n", "aaclip_metrics_pro_curve", ["i0", "i1", N31, "i2", 0.3, "o0", "w", BIG, None],
     "metrics_pro_curve: n must be 2 .. 2^31 - 1", ""),
    ("region_table.n", "aaclip_region_table",
     ["i0", "i1", "i2", "i3", None, 2, 32768, 32768, 1, 16, "o0", "o1", None, "o2", "w", BIG, None],
     "region_table: images, H, W must be positive with 2 .. 2^31 - 1 pixels in all", ""),
    ("support_nearest.M", "aaclip_support_nearest", ["i0", N31, "i1", 16, 64, 0, "o0", "o1", "w", BIG, None],
     "M and N must be 1 .. 2^31 - 1", "support_nearest: "),
    ("support_bank_rows.N", "aaclip_support_bank_rows", ["i0", N31, 64, 0, "o0", None],
     "M and N must be 1 .. 2^31 - 1", "support_bank_rows: "),
    ("coreset_rows.N", "aaclip_coreset_rows", ["i0", N31, 64, "o0", "o1", None], "N must be 1 .. 2^31 - 1", "coreset_rows: "),
    ("coreset_unit_rows.N", "aaclip_coreset_unit_rows", ["i0", N31, 64, "o0", None],
     "N must be 1 .. 2^31 - 1", "coreset_unit_rows: "),
    ("coreset_select.N", "aaclip_coreset_select", ["i0", "i1", N31, 64, 4, 0, "o0", "o1", "o2", "w", BIG, None],
     "N must be 1 .. 2^31 - 1", "coreset_select: "),
]
REFUSAL_SLOT = 4096                                # bytes between the stand-in buffers of a refused call


def refusal_arguments(args, base_in, base_out, base_ws):
    """the ctypes arguments of one refused call: pointer k of a kind lies REFUSAL_SLOT * k into that kind's buffer -> (list
    of arguments, objects that must outlive the call)"""
    import ctypes as C

    from aaclip_hip import _lib
    keep, out = [], []
    for a in args:
        if isinstance(a, str) and a[0] in "io" and a[1:].isdigit():
            out.append((base_in if a[0] == "i" else base_out) + REFUSAL_SLOT * int(a[1:]))
        elif a == "w":
            out.append(base_ws)
        elif a in ("xs", "dxs"):
            arr = (C.c_void_p * 1)((base_in if a == "xs" else base_out) + REFUSAL_SLOT * 7)
            keep.append(arr)
            out.append(C.cast(arr, C.c_void_p))
        elif a == "bw":
            w = _lib.BlockWeights()
            keep.append(w)
            out.append(C.byref(w))
        elif a == "optim":                         # one tensor of one element more than a chunk index can address
            item = (_lib.OptimTensor * 1)()
            item[0].g, item[0].n = base_in, ((1 << 27) - 1) * 16384 + 1
            t = _lib.OptimTensors()
            t.items, t.count = item, 1
            keep += [item, t]
            out.append(C.byref(t))
        elif a == "plan31":
            plan = _lib.BootstrapPlan()
            plan.n, plan.images, plan.replicates = N31, 4, 8
            keep.append(plan)
            out.append(C.byref(plan))
        else:
            out.append(a)
    return out, keep
