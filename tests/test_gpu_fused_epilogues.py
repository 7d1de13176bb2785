"""GPU tests of the forms of the building blocks that only the block path selects (include/aaclip.h, "The block path's
forms of the building blocks"; cases and emulation: tests/fused_epilogue_cases.py), each per element or per byte:

  LayerNorm folding   out16 / stats_out of the residual epilogue, aaclip_ln_stats_finalize, aaclip_adapter_mix_fold,
                      row_ab / col_s of the bias and GELU epilogues (two-set kernels with the pre-K-loop prefetch at
                      K = 128, the one-set kernel at K = 192), and the chain of the three against fp64
  resid               the out-of-place residual read
  split fp16          3-plane (fp16-exact) weights on both tile sizes, every producer of split8 rows with hi8 = false,
                      v's unread lo half, the QKV epilogue's [q k v hi | q8 | k8] records and the attention kernel on them

Row counts 4096 / 4097 / 4225 reach the 256-row-tile kernels with the smallest shapes; 4225 leaves a last tile whose upper
128-row band is full and whose lower band holds one row.  Every case runs under GEMM variants 80 / 81 / 82 (and the
automatic choice) and must give the same bits.  Measured errors go to PARITY_ERRORS under fused.* (committed:
profiles/fused_epilogue_parity_errors.json)."""
import ctypes

import pytest
import torch

import fused_epilogue_cases as FC
from aaclip_hip import _lib, engine, synth
from aaclip_hip._lib import BF16, F16, F16X2, F32
from conftest import PARITY_ERRORS

pytestmark = pytest.mark.gpu

CODE = {"fp16": F16, "bf16": BF16}
VARIANTS = (0, 80, 81, 82)
ATTN_TOL = (4e-4, 1e-3)            # tests/test_gpu_entry_edges.py ATTN_TOL["fp16x2"]
NAN8 = 0x7F                        # e4m3fn NaN


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def variant(lib, v):
    assert lib.aaclip_set_gemm_variant(v) == 0, v


def ptr(t):
    return None if t is None else t.data_ptr()


def assert_close(a, b, atol, rtol, what=""):
    a, b = a.detach().double(), b.detach().double().to(a.device)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.isfinite(a).all(), f"{what}: non-finite output"
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    assert not bad.any(), (f"{what}: {int(bad.sum())}/{bad.numel()} outside {atol}+{rtol}*|ref|; "
                           f"max err {err.max().item():.3e} at ref {b.flatten()[err.argmax()].item():.3e}")


def bits(t):
    """any tensor -> its bytes, for comparisons that must not be fooled by NaN != NaN"""
    return t.contiguous().view(torch.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def sentinel(dev, shape, dtype):
    """a buffer of 0xAA bytes: a negative, non-round value in every format"""
    n = 1
    for d in shape:
        n *= d
    return torch.full((n * torch.empty(0, dtype=dtype).element_size(),), 0xAA, dtype=torch.uint8, device=dev).view(dtype).reshape(shape)


def untouched(t):
    return bool((bits(t) == 0xAA).all())


def fused(lib, dev, code, epi, A, lda, W, bias, out, ldc, M, N, K, act=0, scale_cols=0, scale=1.0, **fields):
    f = _lib.GemmFusedArgs()
    for k, v in fields.items():
        setattr(f, k, v.data_ptr() if torch.is_tensor(v) else v)
    _lib.check(lib.aaclip_gemm_fused(code, epi, A.data_ptr(), lda, W.data_ptr(), ptr(bias), out.data_ptr(), ldc, M, N, K,
                                     act, scale_cols, scale, ctypes.byref(f), stream(dev)), "gemm_fused")


def plain_gemm(lib, dev, code, epi, A, W, bias, out, M, N, K, act=0, scale_cols=0, scale=1.0):
    _lib.check(lib.aaclip_gemm(code, epi, A.data_ptr(), K, W.data_ptr(), ptr(bias), out.data_ptr(), N, M, N, K, act,
                               scale_cols, scale, stream(dev)), "gemm")


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm folding, producer side: the residual epilogue's out16 / stats_out (and resid)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", FC.WIDTHS)
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_resid_epilogue_out16_and_slice_statistics(dev, dtype, N):
    """EPI_BIAS_RESID with out16 + stats_out, in place and with `resid`: the fp32 rows are bit-equal to the call without
    the fold fields; out16 is bit-equal to their 16-bit rounding; every (sum, sumsq) slot of every live row is written and
    is within 64 * 2^-24 * sum|r| (sum r^2) -- the worst case of ANY order of a 64-term fp32 sum -- of the fp64 sums of the
    rounded values; rows >= M of every output and the whole of `resid` stay untouched; all kernel forms give the same bits."""
    lib = _lib.load()
    code, tdt = CODE[dtype], FC.TDT[dtype]
    slots = N // 64
    worst = [0.0, 0.0]
    for K in (128, 192):                      # two-set kernels / the one-set kernel (odd K-tile count)
        W = synth.randn(f"fused.r.w.{N}.{K}", (N, K), K ** -0.5, 2).to(dev).to(tdt)
        bias = synth.randn(f"fused.r.b.{N}", (N,), 0.5, 2).to(dev)
        for M in FC.GEMM_ROWS:
            A = synth.randn(f"fused.r.a.{K}", (4225, K), 1.0, 2)[:M].to(dev).to(tdt)
            x0 = synth.randn(f"fused.r.x.{N}", (4225, N), 2.0, 2, 0.7)[:M].to(dev)
            base = x0.clone()
            plain_gemm(lib, dev, code, _lib.EPI_BIAS_RESID, A, W, bias, base, M, N, K)
            want16 = base.to(tdt)
            r = want16.double().view(M, slots, 64)
            s64, q64, sa = r.sum(-1), (r * r).sum(-1), r.abs().sum(-1)
            try:
                for with_resid in (False, True):
                    for v in VARIANTS:
                        variant(lib, v)
                        out = torch.full((M + 3, N), 7.5, dtype=torch.float32, device=dev)
                        o16 = sentinel(dev, (M + 3, N), tdt)
                        st = sentinel(dev, (M + 3, slots, 2), torch.float32)
                        if with_resid:
                            res = x0.clone()
                            fused(lib, dev, code, _lib.EPI_BIAS_RESID, A, K, W, bias, out, N, M, N, K, resid=res, out16=o16,
                                  stats_out=st)
                            assert torch.equal(res, x0), "resid was modified"
                        else:
                            out[:M] = x0
                            fused(lib, dev, code, _lib.EPI_BIAS_RESID, A, K, W, bias, out, N, M, N, K, out16=o16, stats_out=st)
                        what = f"{dtype} {(M, N, K)} resid={with_resid} variant {v}"
                        assert torch.equal(out[:M], base), f"{what}: fp32 rows differ from the call without the fold fields"
                        assert bool((out[M:] == 7.5).all()) and untouched(o16[M:]) and untouched(st[M:]), f"{what}: rows >= M written"
                        assert same_bits(o16[:M], want16), f"{what}: out16 is not the 16-bit rounding of the fp32 rows"
                        got = st[:M].double()
                        assert torch.isfinite(got).all() and not bool((bits(st[:M].contiguous()).view(torch.int32) == -1431655766).any()), \
                            f"{what}: a statistics slot was not written"
                        es, eq = (got[..., 0] - s64).abs(), (got[..., 1] - q64).abs()
                        tol = 64 * 2.0 ** -24
                        assert bool((es <= tol * sa).all()) and bool((eq <= tol * q64).all()), \
                            (what, float((es / sa).max()), float((eq / q64).max()))
                        worst = [max(worst[0], float((es / sa).max())), max(worst[1], float((eq / q64).max()))]
            finally:
                variant(lib, 0)
    PARITY_ERRORS[f"fused.resid_stats.{dtype}.N{N}"] = {"sum_rel_to_abs_sum": worst[0], "sumsq_rel": worst[1],
                                                        "bar": 64 * 2.0 ** -24}


@pytest.mark.parametrize("code", [F32, F16, F16X2])
def test_resid_read_on_the_small_kernels(dev, code):
    """`resid` on the 128-tile (fp32: 64-tile) kernels: the same bits as the in-place call, the source untouched"""
    lib = _lib.load()
    M, N, K = 300, 256, 128
    A = synth.randn("fused.rs.a", (M, K), 1.0, 3).to(dev)
    W = synth.randn("fused.rs.w", (N, K), K ** -0.5, 3).to(dev)
    bias = synth.randn("fused.rs.b", (N,), 0.5, 3).to(dev)
    x0 = synth.randn("fused.rs.x", (M, N), 2.0, 3).to(dev)
    if code == F16X2:
        Ad, Wd, lda = engine.split_rows(A), engine.split_rows(W, weight=True), 2 * K
    else:
        Ad, Wd, lda = A.to(engine.torch_dtype(code)), W.to(engine.torch_dtype(code)), K
    base = x0.clone()
    _lib.check(lib.aaclip_gemm(code, _lib.EPI_BIAS_RESID, Ad.data_ptr(), lda, Wd.data_ptr(), bias.data_ptr(), base.data_ptr(),
                               N, M, N, K, 0, 0, 1.0, stream(dev)))
    out = torch.full((M + 3, N), 7.5, dtype=torch.float32, device=dev)
    res = x0.clone()
    fused(lib, dev, code, _lib.EPI_BIAS_RESID, Ad, lda, Wd, bias, out, N, M, N, K, resid=res)
    assert torch.equal(out[:M], base) and bool((out[M:] == 7.5).all()) and torch.equal(res, x0)
    assert_close(base, x0.double() + A.double() @ W.double().t() + bias.double(), 4e-3 if code == F16 else 3e-4, 1e-2 if code == F16 else 1e-4)


# ---------------------------------------------------------------------------------------------------------------------
# (sum, sumsq) -> (rstd, -mean * rstd): aaclip_ln_stats_finalize and aaclip_adapter_mix_fold
# ---------------------------------------------------------------------------------------------------------------------
def check_ab(got, ab64, kappa, what):
    """|d rstd| <= 8 * 2^-24 * kappa * rstd per row, the same scale for b (FC.ab_bounds) -> worst ratios to the bound"""
    assert torch.isfinite(got).all(), f"{what}: non-finite (rstd, b)"
    err = (got.double() - ab64).abs()
    ratio = err / FC.ab_bounds(ab64, kappa)
    assert bool((ratio <= 1.0).all()), (what, [float(x) for x in ratio.amax(0)], float(kappa.max()))
    return [float(x) for x in ratio.amax(0)]


@pytest.mark.parametrize("D", FC.WIDTHS)
def test_ln_stats_finalize_every_row_kind(dev, D):
    """Partials of every row kind (fp32 slice sums of fp16- and bf16-rounded rows) -> (rstd, -mean * rstd) against fp64 on
    the SAME partials, inside the kappa bound that the CPU emulation holds; 1, 15, 16, 17 and 4097 rows (16 lanes per
    row, 256 threads per workgroup); rows past the last stay untouched."""
    lib = _lib.load()
    rec = {}
    for kind in FC.KINDS:
        x = FC.rows(kind, 4097, D).to(dev)
        for dtype in ("fp16", "bf16"):
            part = FC.slice_stats_emulated(FC.round16(x, dtype))
            ab64, kappa = FC.finalize64(part, D)
            for R in FC.FIN_ROWS:
                ab = sentinel(dev, (R + 3, 2), torch.float32)
                p = part[:R].contiguous()
                _lib.check(lib.aaclip_ln_stats_finalize(p.data_ptr(), ab.data_ptr(), R, D, FC.EPS, stream(dev)))
                assert untouched(ab[R:]), (kind, dtype, R)
                worst = check_ab(ab[:R], ab64[:R], kappa[:R], f"finalize {kind} {dtype} D{D} rows {R}")
            rec[f"{kind}.{dtype}"] = {"rstd_over_bound": worst[0], "b_over_bound": worst[1], "kappa": float(kappa.max())}
    PARITY_ERRORS[f"fused.finalize.D{D}"] = rec


@pytest.mark.parametrize("D", FC.WIDTHS)
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_adapter_mix_fold_every_row_kind(dev, dtype, D):
    """aaclip_adapter_mix_fold: x bit-equal to aaclip_adapter_mix, out16 bit-equal to its 16-bit rounding, and (rstd, b)
    of those rounded rows against fp64 inside the kappa bound; the row counts of the finalize test."""
    lib = _lib.load()
    tdt = FC.TDT[dtype]
    rec = {}
    for kind in FC.KINDS:
        x0 = FC.rows(kind, 4097, D).to(dev)
        a0 = synth.randn(f"fused.mix.a.{D}", (4097, D), 0.3, 5).to(dev)
        for R in FC.FIN_ROWS:
            want = x0[:R].clone()
            _lib.check(lib.aaclip_adapter_mix(want.data_ptr(), a0.data_ptr(), R, D, 0.1, stream(dev)))
            x = torch.full((R + 3, D), 7.5, dtype=torch.float32, device=dev)
            x[:R] = x0[:R]
            o16 = sentinel(dev, (R + 3, D), tdt)
            ab = sentinel(dev, (R + 3, 2), torch.float32)
            _lib.check(lib.aaclip_adapter_mix_fold(CODE[dtype], x.data_ptr(), a0.data_ptr(), R, D, 0.1, o16.data_ptr(),
                                                   ab.data_ptr(), stream(dev)))
            what = f"adapter_mix_fold {kind} {dtype} D{D} rows {R}"
            assert torch.equal(x[:R], want), f"{what}: x differs from aaclip_adapter_mix"
            assert bool((x[R:] == 7.5).all()) and untouched(o16[R:]) and untouched(ab[R:]), f"{what}: rows past the last written"
            assert same_bits(o16[:R], want.to(tdt)), f"{what}: out16 is not the rounding of x"
            ab64, kappa = FC.finalize64(FC.slice_stats64(o16[:R])[0], D)
            worst = check_ab(ab[:R], ab64, kappa, what)
        rec[kind] = {"rstd_over_bound": worst[0], "b_over_bound": worst[1], "kappa": float(kappa.max())}
    PARITY_ERRORS[f"fused.adapter_mix_fold.{dtype}.D{D}"] = rec


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm folding, consumer side: row_ab / col_s
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_row_ab_col_s_exact_integers(dev, dtype):
    """Integers for the accumulator, the column sums and the bias, powers of two for a and b: a_m acc + b_m s_n + bias_n
    is exact in fp32, so the bias epilogue (with the q scaling on the first 64 columns) must be bit-equal to the rounding
    of the fp64 value, and the GELU epilogue bit-equal to the plain product whose operands carry a_m and b_m s_n in 64
    extra K columns (same fp32 input to the same GELU routine).  K = 128: the two-set kernels with the prefetch of row_ab
    before the K loop; K = 192: the one-set kernel that reads it in the epilogue.  Every row has its own (a, b), so a pair
    read for the wrong row -- the clamped rows of the ragged last tile included -- changes the output; row_ab holds NaN
    past row M - 1."""
    lib = _lib.load()
    code, tdt = CODE[dtype], FC.TDT[dtype]
    g = torch.Generator().manual_seed(7)
    for N in (256, 512):
        for K in (128, 192):
            W = torch.randint(-2, 3, (N, K), generator=g).float()
            s = torch.randint(-4, 5, (N,), generator=g).float()
            bias = torch.randint(-3, 4, (N,), generator=g).float()
            for M in FC.GEMM_ROWS:
                A = torch.randint(-3, 4, (M, K), generator=g).float()
                m = torch.arange(M)
                a = 2.0 ** ((m % 5) - 2).float()
                b = (1 - 2 * ((m // 5) % 2)).float() * 2.0 ** ((m % 3) - 1).float()
                val = a.double()[:, None] * (A.double() @ W.double().t()) + b.double()[:, None] * s.double()[None, :]
                ref = val + bias.double()
                ref[:, :64] *= 0.125
                want_bias = ref.float().to(tdt).to(dev)
                # the same pre-activation from a plain product: A' = [a A | b | 0 ...], W' = [W | s | 0 ...]
                A2 = torch.zeros(M, K + 64)
                A2[:, :K] = a[:, None] * A
                A2[:, K] = b
                W2 = torch.zeros(N, K + 64)
                W2[:, :K] = W
                W2[:, K] = s
                Ad, Wd, A2d, W2d = (t.to(dev).to(tdt) for t in (A, W, A2, W2))
                assert torch.equal(A2d.float().cpu(), A2) and torch.equal(W2d.float().cpu(), W2)      # exact in 16 bits
                bd, sd = bias.to(dev), s.to(dev)
                rowab = torch.full((M + 3, 2), float("nan"), device=dev)
                rowab[:M, 0], rowab[:M, 1] = a.to(dev), b.to(dev)
                want_gelu = torch.empty(M, N, dtype=tdt, device=dev)
                plain_gemm(lib, dev, code, _lib.EPI_BIAS_GELU, A2d, W2d, bd, want_gelu, M, N, K + 64)
                assert_close(want_gelu.float(), FC.gelu64(val + bias.double()), FC.ET[dtype], FC.ET[dtype], "augmented gelu")
                try:
                    for v in VARIANTS:
                        variant(lib, v)
                        what = f"{dtype} {(M, N, K)} variant {v}"
                        out = sentinel(dev, (M + 3, N), tdt)
                        fused(lib, dev, code, _lib.EPI_BIAS, Ad, K, Wd, bd, out, N, M, N, K, scale_cols=64, scale=0.125,
                              row_ab=rowab, col_s=sd)
                        assert same_bits(out[:M], want_bias), f"{what}: folded bias epilogue is not exact"
                        assert untouched(out[M:]), f"{what}: rows >= M written"
                        out = sentinel(dev, (M + 3, N), tdt)
                        fused(lib, dev, code, _lib.EPI_BIAS_GELU, Ad, K, Wd, bd, out, N, M, N, K, row_ab=rowab, col_s=sd)
                        assert same_bits(out[:M], want_gelu), f"{what}: folded GELU epilogue differs from the plain product"
                        assert untouched(out[M:]), f"{what}: rows >= M written"
                finally:
                    variant(lib, 0)


CANCELLING = ("mean8", "mean30", "constant")


@pytest.mark.parametrize("D", FC.WIDTHS)
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_folded_chain_against_fp64_and_the_layernorm_route(dev, dtype, D):
    """The chain the block runs -- residual epilogue with out16 / stats_out -> finalize -> GELU product with row_ab /
    col_s -- on each row kind, against fp64 gelu(LN(x16) W^T + b); the unfused library route (aaclip_layernorm ->
    aaclip_gemm on the same 16-bit rows) against the same reference.  plain, outlier and tiny rows (kappa about 1 or
    below: nothing cancels): both routes inside test_gemm_epilogues' output-rounding bound.  mean8, mean30 and constant
    rows: the folded route within 4 x the error of the CPU emulation of its arithmetic (the rule of the
    cross_rows_levels tests); the LayerNorm route's error is recorded beside it (DESIGN.md 3c discusses the gap)."""
    lib = _lib.load()
    code, tdt, et = CODE[dtype], FC.TDT[dtype], FC.ET[dtype]
    M, N2 = 4097, 256
    W, bias, gamma, beta = (t.to(dev) for t in FC.chain_params(D, N2))
    wf, col_s, fb = FC.fold_weights(W, bias, gamma, beta, dtype)
    W16 = W.to(tdt)
    Wp = synth.randn(f"fused.chain.wp.{D}", (D, 128), 128 ** -0.5, 12).to(dev).to(tdt)
    zero_b = torch.zeros(D, device=dev)
    rec = {}
    for kind in FC.KINDS:
        # the residual product adds a small live term (none on constant rows, which must stay constant)
        Ap = synth.randn(f"fused.chain.ap.{kind}", (M, 128), 0.0 if kind == "constant" else 0.05, 12).to(dev).to(tdt)
        x = FC.rows(kind, M, D).to(dev)
        x16 = sentinel(dev, (M + 3, D), tdt)
        st = sentinel(dev, (M + 3, D // 64, 2), torch.float32)
        ab = sentinel(dev, (M + 3, 2), torch.float32)
        fused(lib, dev, code, _lib.EPI_BIAS_RESID, Ap, 128, Wp, zero_b, x, D, M, D, 128, out16=x16, stats_out=st)
        _lib.check(lib.aaclip_ln_stats_finalize(st.data_ptr(), ab.data_ptr(), M, D, FC.EPS, stream(dev)))
        out = sentinel(dev, (M + 3, N2), tdt)
        fused(lib, dev, code, _lib.EPI_BIAS_GELU, x16, D, wf, fb, out, N2, M, N2, D, row_ab=ab, col_s=col_s)
        assert untouched(out[M:]) and untouched(ab[M:])
        rows16 = x16[:M].float()
        assert same_bits(x16[:M], x[:M].to(tdt))
        if kind == "constant":
            assert bool((rows16 == 2.5).all())
        ab64, kappa = FC.finalize64(FC.slice_stats64(rows16)[0], D)
        check_ab(ab[:M], ab64, kappa, f"chain finalize {kind} {dtype} D{D}")
        ref = FC.chain_reference64(rows16, W, bias, gamma, beta, True)
        # the unfused route on the same rows
        h = torch.empty(M, D, dtype=tdt, device=dev)
        _lib.check(lib.aaclip_layernorm(rows16.data_ptr(), gamma.data_ptr(), beta.data_ptr(), h.data_ptr(), code, M, D, FC.EPS,
                                        stream(dev)))
        out_ln = torch.empty(M, N2, dtype=tdt, device=dev)
        plain_gemm(lib, dev, code, _lib.EPI_BIAS_GELU, h, W16, bias, out_ln, M, N2, D)
        r16 = rows16.cpu()      # the emulation runs on the host: torch's fp32 CPU matmul, no device GEMM in the yardstick
        emu = FC.folded_emulated(r16, FC.finalize_emulated(FC.slice_stats_emulated(r16), D), wf.cpu(), col_s.cpu(), fb.cpu(),
                                 True).to(tdt)
        e_hip = float((out[:M].double() - ref).abs().max())
        e_ln = float((out_ln.double() - ref).abs().max())
        e_emu = float((emu.double() - ref.cpu()).abs().max())
        rec[kind] = {"e_hip": e_hip, "e_emulation": e_emu, "e_layernorm_route": e_ln, "kappa": float(kappa.max())}
        print(f"chain {dtype} D{D} {kind}: folded {e_hip:.3e} emulation {e_emu:.3e} layernorm route {e_ln:.3e} "
              f"kappa {float(kappa.max()):.3g}")
        assert torch.isfinite(out[:M].float()).all()
        if kind in CANCELLING:
            assert e_hip <= 4 * e_emu, (kind, dtype, D, e_hip, e_emu)
        else:
            assert_close(out[:M].float(), ref, et, et, f"folded route {kind} {dtype} D{D}")
            assert_close(out_ln.float(), ref, et, et, f"layernorm route {kind} {dtype} D{D}")
    PARITY_ERRORS[f"fused.chain.{dtype}.D{D}"] = rec


# ---------------------------------------------------------------------------------------------------------------------
# split fp16: 3-plane weights, rows without their hi8 plane, v's unread lo half
# ---------------------------------------------------------------------------------------------------------------------
def planes(rows, K, hi=None, p8a=None, p8b=None, exact=False):
    """hand-built split8 rows from explicit planes: fp16 values, bytes of plane 1, bytes of plane 2 (None = zeros;
    exact: no plane 2 -- the 3-plane weight)"""
    z16 = torch.zeros(rows, K, dtype=torch.float16)
    z8 = torch.zeros(rows, K, dtype=torch.uint8)
    parts = [(hi if hi is not None else z16).contiguous().view(torch.uint8).reshape(rows, 2 * K), p8a if p8a is not None else z8]
    if not exact:
        parts.append(p8b if p8b is not None else z8)
    return torch.cat(parts, dim=1).contiguous()


def e4m3(t):
    return t.float().to(torch.float8_e4m3fn).view(torch.uint8)


def split_gemm(lib, dev, A, W, out, M, N, K, exact):
    """fp32-out split product (no activation) through aaclip_gemm_fused"""
    fused(lib, dev, F16X2, _lib.EPI_ACT_F32, A, 2 * K, W, None, out, N, M, N, K, w_exact16=1 if exact else 0)


@pytest.mark.parametrize("M", [200, 4300])      # 128-tile kernel / 256-tile kernels
def test_three_plane_weights_exact_integers(dev, M):
    """Small integers, K = 256: the 3-plane weight gives the exact product, bit-equal to the 4-plane run with a zero lo
    plane; the integers carried ONLY by the activation's lo8 plane against the weight's e4m3 hi plane (tile T1) still
    arrive -- a correction plane that contributed nothing would give zeros; carried ONLY by the activation's hi8 plane
    they meet no weight plane at all (tile T2 is skipped) -- exactly zero, whatever the 4-plane run does with them."""
    lib = _lib.load()
    N, K = 256, 256
    g = torch.Generator().manual_seed(5)
    A = torch.randint(-3, 4, (M, K), generator=g).float()
    W = torch.randint(-2, 3, (N, K), generator=g).float()
    A[:, 0] += torch.arange(M).float() % 5
    W[:, 1] += torch.arange(N).float() % 3
    ref = (A.double() @ W.double().t()).to(dev)
    As = engine.split_rows(A.to(dev))
    W4, W3 = engine.split_rows(W.to(dev), weight=True), engine.split_rows(W.to(dev), weight=True, exact=True)
    assert W3.shape == (N, 3 * K) and torch.equal(W4[:, :3 * K], W3) and not bool(W4[:, 3 * K:].any())
    A1 = planes(M, K, p8a=e4m3(A)).to(dev)
    W1 = planes(N, K, p8a=e4m3(W * 64), exact=True).to(dev)
    A2 = planes(M, K, p8b=e4m3(A)).to(dev)
    try:
        for v in VARIANTS if M >= 4096 else (0,):
            variant(lib, v)
            out4 = torch.full((M + 3, N), 7.5, dtype=torch.float32, device=dev)
            out3 = out4.clone()
            split_gemm(lib, dev, As, W4, out4, M, N, K, False)
            split_gemm(lib, dev, As, W3, out3, M, N, K, True)
            assert torch.equal(out3[:M].double(), ref), f"variant {v}: 3-plane product is not exact"
            assert torch.equal(out3, out4), f"variant {v}: 3-plane and 4-plane runs differ"
            assert bool((out3[M:] == 7.5).all())
            split_gemm(lib, dev, A1, W1, out3, M, N, K, True)
            assert torch.equal(out3[:M].double() * 1024.0, ref), f"variant {v}: tile T1 of the 3-plane form"
            split_gemm(lib, dev, A2, W3, out3, M, N, K, True)
            assert not bool(out3[:M].any()), f"variant {v}: the 3-plane form read the activation's hi8 plane"
    finally:
        variant(lib, 0)


def consumer_is_blind_to_hi8(lib, dev, full, nohi8, C, what):
    """full / nohi8: split8 rows [R, 4C] bytes of the hi8 = true / false runs.  The hi8 plane of `nohi8` kept its 0xAA
    sentinel in every row, the other planes are bit-identical, and a product with a 3-plane weight returns bit-identical,
    finite results when that plane holds e4m3 NaN bytes."""
    R = full.shape[0]
    full, nohi8 = bits(full).reshape(R, 4 * C), bits(nohi8).reshape(R, 4 * C)
    assert bool((nohi8[:, 3 * C:] == 0xAA).all()), f"{what}: the hi8 plane was written"
    assert torch.equal(nohi8[:, :3 * C], full[:, :3 * C]), f"{what}: hi / lo8 planes differ from the hi8 = true run"
    assert not bool((full[:, 3 * C:] == 0xAA).all()), f"{what}: the hi8 = true run wrote no hi8 plane"
    poisoned = nohi8.clone()
    poisoned[:, 3 * C:] = NAN8
    N = 256
    W3 = engine.split_rows(synth.randn(f"fused.cons.w.{C}", (N, C), C ** -0.5, 8).half().float().to(dev), weight=True, exact=True)
    a, b = (torch.empty(R, N, dtype=torch.float32, device=dev) for _ in range(2))
    split_gemm(lib, dev, full.contiguous(), W3, a, R, N, C, True)
    split_gemm(lib, dev, poisoned, W3, b, R, N, C, True)
    assert torch.isfinite(b).all() and torch.equal(a, b), f"{what}: the consumer read the hi8 plane"
    assert float(a.abs().max()) > 0.1


@pytest.mark.parametrize("M", [200, 4225])      # 128-tile kernel / 256-tile kernels, ragged last tile
def test_gelu_epilogue_without_hi8(dev, M):
    lib = _lib.load()
    N, K = 256, 128
    A = engine.split_rows(synth.randn("fused.g8.a", (M, K), 1.0, 6).to(dev))
    W = engine.split_rows(synth.randn("fused.g8.w", (N, K), K ** -0.5, 6).to(dev), weight=True)
    bias = synth.randn("fused.g8.b", (N,), 0.5, 6).to(dev)
    try:
        for v in VARIANTS if M >= 4096 else (0,):
            variant(lib, v)
            full, no8 = (sentinel(dev, (M + 3, 4 * N), torch.uint8) for _ in range(2))
            plain = full.clone()
            _lib.check(lib.aaclip_gemm(F16X2, _lib.EPI_BIAS_GELU, A.data_ptr(), 2 * K, W.data_ptr(), bias.data_ptr(),
                                       plain.data_ptr(), 2 * N, M, N, K, 0, 0, 1.0, stream(dev)))
            fused(lib, dev, F16X2, _lib.EPI_BIAS_GELU, A, 2 * K, W, bias, full, 2 * N, M, N, K)
            fused(lib, dev, F16X2, _lib.EPI_BIAS_GELU, A, 2 * K, W, bias, no8, 2 * N, M, N, K, out_no_hi8=1)
            assert torch.equal(full, plain) and untouched(no8[M:]) and untouched(full[M:])
            consumer_is_blind_to_hi8(lib, dev, full[:M], no8[:M], N, f"gelu M={M} variant {v}")
    finally:
        variant(lib, 0)


@pytest.mark.parametrize("D", FC.WIDTHS)
def test_layernorm_and_split_rows_without_hi8(dev, D):
    lib = _lib.load()
    R = 37
    x = synth.randn("fused.ln8.x", (R, D), 3.0, 1, mean=0.7).to(dev)
    w, b = synth.randn("fused.ln8.w", (D,), 0.2, 1, 1.0).to(dev), synth.randn("fused.ln8.b", (D,), 0.2, 1).to(dev)
    plain, full, no8 = (sentinel(dev, (R + 3, 4 * D), torch.uint8) for _ in range(3))
    _lib.check(lib.aaclip_layernorm(x.data_ptr(), w.data_ptr(), b.data_ptr(), plain.data_ptr(), F16X2, R, D, 1e-5, stream(dev)))
    for hi8, out in ((1, full), (0, no8)):
        _lib.check(lib.aaclip_layernorm_split(x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), R, D, 1e-5, hi8, stream(dev)))
    assert torch.equal(full, plain) and untouched(no8[R:])
    consumer_is_blind_to_hi8(lib, dev, full[:R], no8[:R], D, f"layernorm D={D}")
    full, no8 = (sentinel(dev, (R + 3, 4 * D), torch.uint8) for _ in range(2))
    for hi8, out in ((1, full), (0, no8)):
        _lib.check(lib.aaclip_split_rows(x.data_ptr(), out.data_ptr(), R, D, hi8, stream(dev)))
    assert torch.equal(full[:R], engine.split_rows(x)) and untouched(full[R:]) and untouched(no8[R:])
    consumer_is_blind_to_hi8(lib, dev, full[:R], no8[:R], D, f"split_rows D={D}")


@pytest.mark.parametrize("cfg", [(2, 77, 4, 1, 0), (1, 640, 4, 0, 0), (1, 513, 4, 0, 1)])   # B, L, H, causal, qk8
def test_attention_context_without_hi8(dev, cfg):
    """the context rows of the short-row kernel, the long-row kernel and the e4m3 record form with hi8 = false"""
    lib = _lib.load()
    B, L, H, causal, qk8 = cfg
    D = 64 * H
    qkv = FC.attention_inputs(B, H, L)
    qd = (FC.qk8_records(qkv, H) if qk8 else engine.split16_rows(qkv)).to(dev)
    plain, full, no8 = (sentinel(dev, (B * L + 3, 4 * D), torch.uint8) for _ in range(3))
    if not qk8:
        _lib.check(lib.aaclip_attention_log2q(F16X2, qd.data_ptr(), plain.data_ptr(), B, L, H, causal, stream(dev)))
    for hi8, out in ((1, full), (0, no8)):
        _lib.check(lib.aaclip_attention_split(qd.data_ptr(), out.data_ptr(), B, L, H, causal, 1, qk8, hi8, stream(dev)))
    assert qk8 or torch.equal(full, plain)
    assert untouched(full[B * L:]) and untouched(no8[B * L:])
    consumer_is_blind_to_hi8(lib, dev, full[:B * L], no8[:B * L], D, f"attention {cfg}")


@pytest.mark.parametrize("log2q", [0, 1])
def test_long_row_attention_never_reads_v_lo(dev, log2q):
    """split16 rows at L >= 512: v's lo half is read by nobody -- fp16 NaN there leaves the context bit-identical"""
    lib = _lib.load()
    B, L, H = 2, 513, 2
    D = 64 * H
    qkv = FC.attention_inputs(B, H, L)
    qd = engine.split16_rows(qkv).to(dev)
    bad = qd.clone()
    bad[:, 5 * D:] = float("nan")
    a, b = (sentinel(dev, (B * L, 4 * D), torch.uint8) for _ in range(2))
    _lib.check(lib.aaclip_attention_split(qd.data_ptr(), a.data_ptr(), B, L, H, 0, log2q, 0, 1, stream(dev)))
    _lib.check(lib.aaclip_attention_split(bad.data_ptr(), b.data_ptr(), B, L, H, 0, log2q, 0, 1, stream(dev)))
    assert torch.equal(a, b) and torch.isfinite(engine.join_split8(b, D)).all()


# ---------------------------------------------------------------------------------------------------------------------
# the QKV epilogue's attention records (out_qk8) and the attention kernel on them
# ---------------------------------------------------------------------------------------------------------------------
def qk8_gemm(lib, dev, A, W, bias, out, ldc, M, N, K, out_qk8, scale_cols, scale, exact=0):
    fused(lib, dev, F16X2, _lib.EPI_BIAS, A, 2 * K, W, bias, out, ldc, M, N, K, scale_cols=scale_cols, scale=scale,
          out_qk8=out_qk8, w_exact16=exact)


@pytest.mark.parametrize("shape", [(768, 512, 128), (256, 128, 256), (256, 256, 128)])      # N, out_qk8, K
def test_out_qk8_records_byte_for_byte(dev, shape):
    """A product whose outputs are exactly hi + lo8 * 2^-10: A entries in {0, 1} (at most three per row), W entries in
    {0, 1, 2^-13}, integer bias -- every output is p + q * 2^-13 with p <= 5, q <= 3, exact in fp32, so every byte of the
    row (fp16 plane, [lo8 | hi8] records, v columns) is the host builder's; nothing is written past N + out_qk8 halves of
    a row, nor in rows >= M.  Row strides N + out_qk8 (what the block passes: 5D for N = 3D) and 16 halves more; at
    K = 256 also with the weight in its 3-plane form (the block's QKV product on a checkpoint stored in fp16)."""
    lib = _lib.load()
    N, Q, K = shape
    g = torch.Generator().manual_seed(11)
    W = torch.tensor([0.0, 1.0, 2.0 ** -13])[torch.randint(0, 3, (N, K), generator=g)]
    bias = torch.randint(0, 3, (N,), generator=g).float()
    Wd, bd = engine.split_rows(W.to(dev), weight=True), bias.to(dev)
    weights = [(Wd, 0)] + ([(engine.split_rows(W.to(dev), weight=True, exact=True), 1)] if K % 256 == 0 else [])
    for M in FC.GEMM_ROWS:
        m = torch.arange(M)
        A = torch.zeros(M, K)
        for mul, add in ((1, 0), (7, 3), (13, 5)):
            A[m, (mul * m + add) % K] = 1.0
        ref = A.double() @ W.double().t() + bias.double()
        ref[:, :64] *= 0.5
        val = ref.float()
        assert torch.equal(val.double(), ref)
        want = FC.qk8_records_cols(val, Q)
        # the construction holds what it promises: hi + lo8 * 2^-10 is the value itself
        s = engine.split_rows(val)
        assert torch.equal(engine.join_split8(s, N), ref) and bool(s[:, 2 * N:3 * N].any())
        Ad = engine.split_rows(A.to(dev))
        row = 2 * N + 2 * Q
        try:
            for pad in (0, 16):
                ldc = N + Q + pad
                for v in VARIANTS:
                    variant(lib, v)
                    for Wx, exact in weights:
                        out = sentinel(dev, (M + 3, 2 * ldc), torch.uint8)
                        qk8_gemm(lib, dev, Ad, Wx, bd, out, ldc, M, N, K, Q, 64, 0.5, exact)
                        what = f"{(M, N, K)} out_qk8 {Q} ldc {ldc} variant {v} exact {exact}"
                        assert torch.equal(out[:M, :2 * N].cpu(), want[:, :2 * N]), f"{what}: fp16 plane"
                        assert torch.equal(out[:M, 2 * N:row].cpu(), want[:, 2 * N:]), f"{what}: e4m3 records"
                        assert untouched(out[:M, row:]) and untouched(out[M:]), f"{what}: bytes past the row / rows >= M written"
        finally:
            variant(lib, 0)


@pytest.fixture(scope="module")
def qkv_records(dev):
    """The QKV product as the block runs it, N = 768 (D = 256, H = 4), out_qk8 = 512, M = 4225 = 5 images of 845 rows,
    random data -> (records [M, 10 D] bytes, fp64 reference of the product), written once under every kernel form"""
    lib = _lib.load()
    M, N, K, Q = 4225, 768, 256, 512
    A = synth.randn("fused.qk.a", (M, K), 1.0, 2)
    W = synth.randn("fused.qk.w", (N, K), K ** -0.5, 2)
    bias = synth.randn("fused.qk.b", (N,), 0.5, 2)
    Ad, Wd, bd = engine.split_rows(A.to(dev)), engine.split_rows(W.to(dev), weight=True), bias.to(dev)
    ref = A.double() @ W.double().t() + bias.double()
    ref[:, :256] *= 0.125 * 1.4426950408889634
    outs = []
    try:
        for v in VARIANTS:
            variant(lib, v)
            out = sentinel(dev, (M + 3, 2 * (N + Q)), torch.uint8)
            qk8_gemm(lib, dev, Ad, Wd, bd, out, N + Q, M, N, K, Q, 256, 0.125 * 1.4426950408889634)
            outs.append(out)
    finally:
        variant(lib, 0)
    for o in outs[1:]:
        assert torch.equal(o, outs[0]), "the kernel forms write different records"
    assert untouched(outs[0][M:])
    return outs[0][:M].contiguous(), ref


def test_out_qk8_records_random_data(dev, qkv_records):
    """q and k: hi + lo8 * 2^-10 within test_gemm_split_epilogues' 3e-4 + 1e-4 |ref| of fp64, hi8 within 2^-4 relative
    (2^-9 absolute) as test_layernorm_split_output asserts; v: one fp16 rounding (2^-11 relative) on top of the product's
    bound -- it carries no correction."""
    rec, ref = qkv_records
    H, D = 4, 256
    joined = FC.qk8_join(rec, H)
    assert_close(joined[:, :2 * D], ref[:, :2 * D], 3e-4, 1e-4, "q | k records")
    assert_close(joined[:, 2 * D:], ref[:, 2 * D:], 3e-4, 1e-4 + 2.0 ** -11, "v columns")
    _, _, hi8 = FC.qk8_planes(rec, H)
    h = hi8.view(torch.float8_e4m3fn).double()
    r = ref[:, :2 * D]
    worst = float(((h - r).abs() / (r.abs() * 2.0 ** -4 + 2.0 ** -9)).max())
    assert worst <= 1.0, worst
    e = (joined - ref).abs()
    PARITY_ERRORS["fused.out_qk8.random"] = {"qk_max_abs_err": float(e[:, :2 * D].max()), "v_max_abs_err": float(e[:, 2 * D:].max()),
                                             "hi8_over_bound": worst}


def run_qk8(lib, dev, rec, B, L, H):
    ctx = sentinel(dev, (B * L + 3, 256 * H), torch.uint8)
    r = rec.to(dev)
    _lib.check(lib.aaclip_attention_split(r.data_ptr(), ctx.data_ptr(), B, L, H, 0, 1, 1, 1, stream(dev)), "attention_split")
    assert untouched(ctx[B * L:])
    return engine.join_split8(ctx[:B * L], 64 * H)


def run_split16(lib, dev, seen, B, L, H):
    ctx = sentinel(dev, (B * L + 3, 256 * H), torch.uint8)
    q = engine.split16_rows(seen.float()).to(dev)
    _lib.check(lib.aaclip_attention_split(q.data_ptr(), ctx.data_ptr(), B, L, H, 0, 1, 0, 1, stream(dev)), "attention_split")
    assert untouched(ctx[B * L:])
    return engine.join_split8(ctx[:B * L], 64 * H)


def worst_ratio(got, ref, atol, rtol):
    return float(((got - ref).abs() / (atol + rtol * ref.abs())).max())


@pytest.mark.parametrize("cfg", FC.QK8_ATTENTION_CASES)
def test_qk8_attention_on_host_built_records(dev, cfg):
    """The e4m3 record form against fp64 attention of the values the records hold (q, k = hi + lo8 * 2^-10, v = hi), at
    ATTN_TOL['fp16x2']; the split16 form of the SAME values inside the same bound; and the records with their correction
    planes zeroed -- all of them, then only the operands of one of the two e4m3 products -- each further from the reference
    than the full records: both products contribute."""
    lib = _lib.load()
    B, H, L = cfg
    D = 64 * H
    rec = FC.qk8_records(FC.attention_inputs(B, H, L), H)
    seen = FC.qk8_join(rec, H)
    assert torch.equal(seen.float().double(), seen)                    # the joined values are exact in fp32
    ref = FC.attention_reference64(seen, B, L, H)
    got = run_qk8(lib, dev, rec, B, L, H)
    assert_close(got, ref, *ATTN_TOL, f"qk8 attention {cfg}")
    got16 = run_split16(lib, dev, seen, B, L, H)
    assert_close(got16, ref, *ATTN_TOL, f"split16 attention of the same values {cfg}")
    e_full = float((got - ref).abs().max())
    errs = {"full": e_full, "split16": float((got16 - ref).abs().max())}
    # planes of the records: [R, q heads | k heads, lo8 | hi8, 64].  The kernel's two e4m3 products are Kl8.Qh8 and Kh8.Ql8
    for name, dead in (("no_corrections", [(slice(None), slice(None))]),
                       ("without_Kh8_Ql8", [(slice(0, H), 0), (slice(H, 2 * H), 1)]),
                       ("without_Kl8_Qh8", [(slice(0, H), 1), (slice(H, 2 * H), 0)])):
        z = rec.clone()
        planes8 = z[:, 6 * D:].view(B * L, 2 * H, 2, 64)
        for heads, plane in dead:
            planes8[:, heads, plane] = 0
        errs[name] = float((run_qk8(lib, dev, z, B, L, H) - ref).abs().max())
        assert errs[name] > e_full, (cfg, name, errs)
    PARITY_ERRORS[f"fused.qk8_attention.B{B}.H{H}.L{L}"] = errs


def test_qk8_attention_first_tile_far_below_zero(dev):
    """test_attention_first_tile_far_below_zero's rows (every score of the first key tiles at about -150 in log2 units,
    one late key at +4) at L = 700 through the record form, at that test's tolerance for split fp16"""
    lib = _lib.load()
    L, H = 700, 1
    qkv = synth.randn("t.attn.neg", (L, 192), 0.3, 9)
    qkv[:, :64] *= 0.2
    qkv[:, 0] = 1.0
    qkv[:, 64] = -150.0
    qkv[L - 3, 64] = 4.0
    rec = FC.qk8_records(qkv, H)
    ref = FC.attention_reference64(FC.qk8_join(rec, H), 1, L, H)
    got = run_qk8(lib, dev, rec, 1, L, H)
    assert_close(got, ref, 4e-4, 1e-2, "first tile -150, record form")
    PARITY_ERRORS["fused.qk8_attention.first_tile_minus_150.L700"] = float((got - ref).abs().max())


def test_qk8_attention_on_gemm_written_records(dev, qkv_records):
    """end to end: the records the QKV epilogue wrote (5 images of 845 rows, 4 heads) through the attention kernel,
    against fp64 attention of the values those records hold"""
    lib = _lib.load()
    rec, _ = qkv_records
    B, L, H = 5, 845, 4
    ref = FC.attention_reference64(FC.qk8_join(rec, H), B, L, H)
    got = run_qk8(lib, dev, rec, B, L, H)
    assert_close(got, ref, *ATTN_TOL, "attention on GEMM-written records")
    PARITY_ERRORS["fused.qk8_attention.gemm_written.B5.H4.L845"] = float((got - ref).abs().max())
