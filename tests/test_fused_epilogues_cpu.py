"""Host-side checks of the block path's building-block exports (include/aaclip.h, ABI 10) and of the cases in
tests/fused_epilogue_cases.py: no GPU needed -- every argument check of the entry points precedes the first HIP call."""
import ctypes
import os
import re

import pytest
import torch

import fused_epilogue_cases as FC
from aaclip_hip import _lib, engine
from aaclip_hip._lib import BF16, F16, F16X2, F32

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("aaclip_gemm_fused", "aaclip_ln_stats_finalize", "aaclip_adapter_mix_fold", "aaclip_attention_split",
       "aaclip_layernorm_split", "aaclip_split_rows")
# plausible, aligned device addresses: nothing here may be dereferenced
PA, PW, PB, PO, P1, P2, P3 = (0x7f0000001000 + 0x100000 * i for i in range(7))


def test_exports_and_struct_match_the_header():
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "aaclip.h")).read()
    assert "#define AACLIP_ABI_VERSION 10 " in header and lib.aaclip_version() == 10 == _lib.ABI_VERSION
    for name in NEW:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None, name
        assert re.search(r"\b%s\s*\(" % name, header), name
    body = re.search(r"typedef struct aaclip_gemm_fused_args \{(.*?)\} aaclip_gemm_fused_args;", header, re.S).group(1)
    fields = re.findall(r"\b(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [n for n, _ in _lib.GemmFusedArgs._fields_]
    assert _lib.GemmFusedArgs().struct_bytes == ctypes.sizeof(_lib.GemmFusedArgs) == 6 * 8 + 3 * 4 + 4
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in integration, name


def _fused(lib, dtype, epi, M, N, K, lda=None, ldc=None, scale_cols=0, **fields):
    f = _lib.GemmFusedArgs()
    for k, v in fields.items():
        setattr(f, k, v)
    split = dtype == F16X2
    if lda is None:
        lda = 2 * K if split else K
    if ldc is None:
        ldc = 2 * N if split and epi in (_lib.EPI_BIAS, _lib.EPI_BIAS_GELU) else N
    rc = lib.aaclip_gemm_fused(dtype, epi, PA, lda, PW, PB, PO, ldc, M, N, K, 0, scale_cols, 1.0, ctypes.byref(f), None)
    return rc, lib.aaclip_last_error()


def refused(res, word):
    rc, msg = res
    assert rc == -1 and word in msg, (rc, msg)


def test_gemm_fused_refuses_a_struct_of_another_size():
    lib = _lib.load()
    f = _lib.GemmFusedArgs()
    for size in (0, ctypes.sizeof(_lib.GemmFusedArgs) - 8, ctypes.sizeof(_lib.GemmFusedArgs) + 8):
        f.struct_bytes = size
        rc = lib.aaclip_gemm_fused(F16, _lib.EPI_BIAS, PA, 128, PW, PB, PO, 256, 4096, 256, 128, 0, 0, 1.0,
                                   ctypes.byref(f), None)
        assert rc == -1 and b"struct_bytes" in lib.aaclip_last_error(), size
    rc = lib.aaclip_gemm_fused(F16, _lib.EPI_BIAS, PA, 128, PW, PB, PO, 256, 4096, 256, 128, 0, 0, 1.0, None, None)
    assert rc == -1 and b"null argument struct" in lib.aaclip_last_error()


def test_gemm_fused_refuses_fields_the_selected_kernel_does_not_implement():
    """Every field of aaclip_gemm_fused_args on a dtype, epilogue, shape or kernel selection whose kernel would ignore
    it (the 128-tile kernels know nothing of out16 / stats_out / row_ab / col_s / out_qk8)."""
    lib = _lib.load()
    RESID, BIAS, GELU, ACT = _lib.EPI_BIAS_RESID, _lib.EPI_BIAS, _lib.EPI_BIAS_GELU, _lib.EPI_ACT_F32
    fold_out = dict(out16=P1, stats_out=P2)
    fold_in = dict(row_ab=P1, col_s=P2)
    # resid
    refused(_fused(lib, F16, BIAS, 4096, 256, 128, resid=P1), b"resid belongs")
    refused(_fused(lib, F16, RESID, 4096, 256, 128, resid=P1 + 4), b"resid must be 16-byte aligned")
    # out16 / stats_out
    refused(_fused(lib, F16, RESID, 4096, 256, 128, out16=P1), b"given together")
    refused(_fused(lib, F16, RESID, 4096, 256, 128, stats_out=P2), b"given together")
    refused(_fused(lib, F16, BIAS, 4096, 256, 128, **fold_out), b"out16 / stats_out need")
    refused(_fused(lib, F32, RESID, 4096, 256, 128, **fold_out), b"out16 / stats_out need")
    refused(_fused(lib, F16X2, RESID, 4096, 256, 128, **fold_out), b"out16 / stats_out need")
    refused(_fused(lib, BF16, RESID, 4095, 256, 128, **fold_out), b"out16 / stats_out need")     # 128-tile kernel: M
    refused(_fused(lib, F16, RESID, 4096, 384, 128, **fold_out), b"out16 / stats_out need")      # ... N % 256
    refused(_fused(lib, F16, RESID, 4096, 256, 128, ldc=258, **fold_out), b"out16 / stats_out need")   # ... ldc % 8
    refused(_fused(lib, F16, RESID, 4096, 256, 128, out16=P1 + 2, stats_out=P2), b"8-byte aligned")
    # row_ab / col_s
    refused(_fused(lib, F16, GELU, 4096, 256, 128, row_ab=P1), b"given together")
    refused(_fused(lib, F16, GELU, 4096, 256, 128, col_s=P2), b"given together")
    refused(_fused(lib, F16, RESID, 4096, 256, 128, **fold_in), b"row_ab / col_s need")
    refused(_fused(lib, F16, ACT, 4096, 256, 128, **fold_in), b"row_ab / col_s need")
    refused(_fused(lib, F32, BIAS, 4096, 256, 128, **fold_in), b"row_ab / col_s need")
    refused(_fused(lib, F16X2, GELU, 4096, 256, 128, **fold_in), b"row_ab / col_s need")
    refused(_fused(lib, BF16, GELU, 4000, 256, 128, **fold_in), b"row_ab / col_s need")
    refused(_fused(lib, F16, BIAS, 4096, 256, 128, scale_cols=62, **fold_in), b"row_ab / col_s need")   # scale_cols % 4
    refused(_fused(lib, F16, BIAS, 4096, 256, 128, row_ab=P1, col_s=P2 + 8), b"col_s 16-byte aligned")
    # the fold fields under the forced 128-tile kernel (GEMM variant 1), which would silently ignore them
    try:
        assert lib.aaclip_set_gemm_variant(1) == 0
        refused(_fused(lib, F16, RESID, 4096, 256, 128, **fold_out), b"out16 / stats_out need")
        refused(_fused(lib, F16, GELU, 4096, 256, 128, **fold_in), b"row_ab / col_s need")
        refused(_fused(lib, F16X2, BIAS, 4096, 256, 128, ldc=384, out_qk8=128), b"out_qk8 needs")
    finally:
        assert lib.aaclip_set_gemm_variant(0) == 0
    # w_exact16
    refused(_fused(lib, F16, BIAS, 4096, 256, 256, w_exact16=1), b"w_exact16")
    refused(_fused(lib, F16X2, ACT, 200, 256, 384, w_exact16=1), b"w_exact16")                 # K % 256
    refused(_fused(lib, F16X2, ACT, 200, 256, 256, w_exact16=2), b"0 or 1")
    # out_no_hi8
    refused(_fused(lib, F16X2, BIAS, 200, 256, 128, out_no_hi8=1), b"out_no_hi8 belongs")
    refused(_fused(lib, F16, GELU, 200, 256, 128, out_no_hi8=1), b"out_no_hi8 belongs")
    refused(_fused(lib, F16X2, GELU, 200, 256, 128, out_no_hi8=-1), b"0 or 1")
    # out_qk8: the bias epilogue of the split 256-tile kernel; a multiple of 64, <= N; ldc >= N + out_qk8 halves
    refused(_fused(lib, F16X2, GELU, 4096, 256, 128, ldc=512, out_qk8=128), b"out_qk8 needs")
    refused(_fused(lib, F16, BIAS, 4096, 256, 128, out_qk8=128), b"out_qk8 needs")
    refused(_fused(lib, F16X2, BIAS, 4095, 256, 128, ldc=384, out_qk8=128), b"out_qk8 needs")   # 128-tile kernel
    refused(_fused(lib, F16X2, BIAS, 4096, 384, 128, ldc=512, out_qk8=128), b"out_qk8 needs")   # N % 256
    refused(_fused(lib, F16X2, BIAS, 4096, 256, 128, ldc=384, out_qk8=96), b"multiple of 64")
    refused(_fused(lib, F16X2, BIAS, 4096, 256, 128, ldc=640, out_qk8=320), b"at most N")
    refused(_fused(lib, F16X2, BIAS, 4096, 256, 128, ldc=376, out_qk8=128), b"N + out_qk8")
    refused(_fused(lib, F16X2, BIAS, 4096, 768, 128, ldc=768 + 256, out_qk8=512), b"N + out_qk8")   # N + out_qk8 / 2
    refused(_fused(lib, F16X2, BIAS, 4096, 256, 128, ldc=384, out_qk8=-64), b"column count")
    # without out_qk8 the split16 rule still holds
    refused(_fused(lib, F16X2, BIAS, 4096, 256, 128, ldc=384), b"ldc (in halves) must be >= 2N")
    # and aaclip_gemm's own rules come first
    refused(_fused(lib, 7, BIAS, 4096, 256, 128), b"bad dtype")
    refused(_fused(lib, F16, 9, 4096, 256, 128), b"bad epilogue")
    refused(_fused(lib, F16, BIAS, 4096, 200, 128), b"N must be a multiple of 128")


def test_row_entries_refuse_bad_arguments():
    lib = _lib.load()

    def no(rc, word):
        assert rc == -1 and word in lib.aaclip_last_error(), (rc, lib.aaclip_last_error())

    for D in (0, 64, 320, 2048):
        no(lib.aaclip_ln_stats_finalize(P1, P2, 16, D, 1e-5, None), b"row width")
        no(lib.aaclip_adapter_mix_fold(F16, PA, PB, 16, D, 0.1, P1, P2, None), b"row width")
        no(lib.aaclip_layernorm_split(PA, PW, PB, PO, 16, D, 1e-5, 1, None), b"row width")
    no(lib.aaclip_ln_stats_finalize(None, P2, 16, 256, 1e-5, None), b"null pointer")
    no(lib.aaclip_ln_stats_finalize(P1, None, 16, 256, 1e-5, None), b"null pointer")
    no(lib.aaclip_ln_stats_finalize(P1, P2 + 4, 16, 256, 1e-5, None), b"8-byte aligned")
    no(lib.aaclip_ln_stats_finalize(P1, P2, 0, 256, 1e-5, None), b"rows must be")
    no(lib.aaclip_ln_stats_finalize(P1, P2, 1 << 27, 256, 1e-5, None), b"rows must be")
    for dtype in (F32, F16X2, 9):
        no(lib.aaclip_adapter_mix_fold(dtype, PA, PB, 16, 256, 0.1, P1, P2, None), b"fp16 or bf16")
    no(lib.aaclip_adapter_mix_fold(F16, PA, PB, 16, 256, 0.1, None, P2, None), b"bad arguments")
    no(lib.aaclip_adapter_mix_fold(F16, PA, PB, 16, 256, 0.1, P1, None, None), b"bad arguments")
    no(lib.aaclip_adapter_mix_fold(BF16, PA, PB, 0, 256, 0.1, P1, P2, None), b"bad arguments")
    no(lib.aaclip_adapter_mix_fold(BF16, PA + 8, PB, 16, 256, 0.1, P1, P2, None), b"aligned")
    no(lib.aaclip_layernorm_split(PA, PW, PB, None, 16, 256, 1e-5, 0, None), b"null pointer")
    no(lib.aaclip_layernorm_split(PA, PW, PB, PO, 0, 256, 1e-5, 0, None), b"rows must be positive")
    no(lib.aaclip_split_rows(None, PO, 16, 256, 1, None), b"null pointer")
    no(lib.aaclip_split_rows(PA, PO + 8, 16, 256, 1, None), b"16-byte aligned")
    no(lib.aaclip_split_rows(PA, PO, 16, 100, 1, None), b"multiple of 8")
    no(lib.aaclip_split_rows(PA, PO, 0, 256, 1, None), b"multiple of 8")


def test_attention_split_refuses_records_where_the_kernel_does_not_take_them():
    """qk8 records need attention_qk8_applicable (L >= 512, not causal) and q in log2 units"""
    lib = _lib.load()

    def no(rc, word):
        assert rc == -1 and word in lib.aaclip_last_error(), (rc, lib.aaclip_last_error())

    no(lib.aaclip_attention_split(PA, PO, 1, 511, 1, 0, 1, 1, 1, None), b"record form")      # short rows
    no(lib.aaclip_attention_split(PA, PO, 1, 512, 1, 1, 1, 1, 1, None), b"record form")      # causal
    no(lib.aaclip_attention_split(PA, PO, 1, 512, 1, 0, 0, 1, 1, None), b"record form")      # q not in log2 units
    no(lib.aaclip_attention_split(None, PO, 1, 512, 1, 0, 1, 1, 1, None), b"null pointer")
    no(lib.aaclip_attention_split(PA, PO, 0, 512, 1, 0, 1, 0, 1, None), b"empty problem")
    no(lib.aaclip_attention_split(PA, PO, 70000, 512, 1, 0, 1, 0, 1, None), b"grid limit")
    no(lib.aaclip_attention_split(PA, PO, 1, 1 << 20, 4, 0, 1, 0, 1, None), b"2^31")


def test_record_builder_round_trip():
    """qk8_records is engine.split_rows per head: the joined value is split8's (2^-15 relative for q and k, fp16 for v),
    every plane comes back byte for byte, and a row is 10 D bytes."""
    for H in (1, 2, 12):
        D = 64 * H
        qkv = FC.attention_inputs(1, H, 37)
        rec = FC.qk8_records(qkv, H)
        assert rec.dtype == torch.uint8 and rec.shape == (37, 10 * D)
        s = engine.split_rows(qkv)
        hi, lo8, hi8 = FC.qk8_planes(rec, H)
        assert torch.equal(hi.view(torch.uint8).reshape(37, -1), s[:, :6 * D])
        assert torch.equal(lo8, s[:, 6 * D:8 * D]) and torch.equal(hi8, s[:, 9 * D:11 * D])
        # head h of q at record h, of k at record H + h: [lo8 64 B | hi8 64 B]
        for g in (0, H - 1, H, 2 * H - 1):
            r = rec[:, 6 * D + 128 * g:6 * D + 128 * (g + 1)]
            assert torch.equal(r[:, :64], s[:, 6 * D + 64 * g:6 * D + 64 * (g + 1)])
            assert torch.equal(r[:, 64:], s[:, 9 * D + 64 * g:9 * D + 64 * (g + 1)])
        j = FC.qk8_join(rec, H)
        x = qkv.double()
        assert torch.equal(j[:, :2 * D], engine.join_split8(s, 3 * D)[:, :2 * D])
        assert float(((j[:, :2 * D] - x[:, :2 * D]).abs() / (x[:, :2 * D].abs() * 2.0 ** -15 + 2.0 ** -19)).max()) <= 1.0
        assert torch.equal(j[:, 2 * D:], qkv[:, 2 * D:].half().double())
        z = FC.qk8_without_corrections(rec, H)
        assert torch.equal(FC.qk8_join(z, H), hi.double()) and torch.equal(z[:, :6 * D], rec[:, :6 * D])


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("D", FC.WIDTHS)
def test_emulated_finalize_holds_the_kappa_bound_on_every_row_kind(D, dtype):
    """The fp32 emulation of (rstd, -mean * rstd) against fp64 on the same 16-bit rows: inside 8 * 2^-24 * kappa for every
    kind -- the bound the GPU tests put on the kernels.  Also that the kinds are what they claim: kappa spans 1 ... 6e5."""
    for kind in FC.KINDS:
        x16 = FC.round16(FC.rows(kind, 64, D), dtype)
        exact, _ = FC.slice_stats64(x16)
        ab64, kappa = FC.finalize64(exact, D)
        ab = FC.finalize_emulated(FC.slice_stats_emulated(x16), D)
        err = (ab.double() - ab64).abs()
        bound = FC.ab_bounds(ab64, kappa)
        assert torch.isfinite(ab).all() and bool((err <= bound).all()), (kind, D, dtype, float((err / bound).max()))
        k = float(kappa.median())
        lo, hi = {"plain": (1.0, 1.2), "mean8": (40, 100), "mean30": (2000, 5000), "outlier": (1.0, 1.2),
                  "tiny": (0.0, 1.0), "constant": (6e5, 7e5)}[kind]
        assert lo <= k <= hi, (kind, D, dtype, k)
    # beyond the kinds: at mean 100 the bound itself reaches 10 % -- the form has no accuracy left to assert there
    x16 = FC.round16(100.0 + torch.randn(8, D, generator=torch.Generator().manual_seed(1)), "fp16")
    _, kappa = FC.finalize64(FC.slice_stats64(x16)[0], D)
    assert FC.RSTD_BOUND * float(kappa.max()) > 3e-3


def test_emulated_folded_product_matches_the_layernorm_route_on_plain_rows():
    """On plain rows the folded arithmetic is the LayerNorm route up to fp32 rounding: the emulation (before the output
    rounding) is within 2e-5 of fp64 gelu(LN(x16) W^T + b) -- far inside the 1.5e-3 the 16-bit output costs."""
    D, N = 256, 256
    W, bias, gamma, beta = FC.chain_params(D, N)
    x16 = FC.round16(FC.rows("plain", 33, D), "fp16")
    wf, col_s, fb = FC.fold_weights(W, bias, gamma, beta, "fp16")
    ab = FC.finalize_emulated(FC.slice_stats_emulated(x16), D)
    got = FC.folded_emulated(x16, ab, wf, col_s, fb, True).double()
    # reference with the 16-bit folded weight, so that only the arithmetic differs
    ref = FC.gelu64(torch.nn.functional.layer_norm(x16.double(), (D,), None, None, FC.EPS) @ wf.double().t() + fb.double())
    assert float((got - ref).abs().max()) < 2e-5
