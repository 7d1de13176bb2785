"""The fp32 building blocks of csrc/text_backward.hip on the GPU, one kernel at a time and judged per element
(tests/backward_blocks_cases.py holds the shapes, the fp64 references and the bounds, and says where each bound comes
from): the weight-gradient GEMM at every edge of its row chunking, with strides, exact integers and a poisoned
workspace; the LayerNorm, adapter-mix and head-normalize row kernels at the three widths, with the aliasing the block
backward relies on and sentinel rows behind every output; LeakyReLU's derivative at exactly zero; the short attention
backward around its 64-key split.  The C ABI is called through ctypes wherever engine exposes no stride, alias or
oversized buffer.  Every measured figure goes to PARITY_ERRORS under backward_blocks.*"""
import math

import pytest
import torch

import backward_blocks_cases as BB
from aaclip_hip import _lib, engine
from conftest import PARITY_ERRORS
from visual_backward_cases import rel

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def filled(dev, shape, value):
    return torch.full(shape, value, dtype=torch.float32, device=dev)


def with_tail(t, dev, value=NAN):
    """t [rows, D] on the device with BB.TAIL_ROWS rows of `value` behind it (a whole workgroup's worth: a kernel without
    its row guard stays inside the buffer and shows in the tail)"""
    buf = filled(dev, (t.shape[0] + BB.TAIL_ROWS, t.shape[1]), value)
    buf[:t.shape[0]] = t.to(dev)
    return buf


def tail_untouched(buf, rows, value):
    tail = buf[rows:]
    return bool(tail.isnan().all()) if math.isnan(value) else bool((tail == value).all())


def check_bound(key, got, want, terms, K):
    """Every element within K * 2^-24 * terms (an element without terms: exact) -> the largest ratio, recorded"""
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert torch.isfinite(got).all(), key
    r = BB.ratio(got, want, terms)
    print(key, "largest |err| / (2^-24 terms):", r, "of", K)
    PARITY_ERRORS["backward_blocks." + key] = r
    assert r <= K, (key, r, K)
    return r


# ---------------------------------------------------------------------------------------------- gemm_wgrad
def wgrad(dev, dz, ldz, u, ldu, rows, O, I):
    """aaclip_gemm_wgrad on device operands (tensors or (buffer, element offset) windows) with a NaN-filled workspace
    and a sentinel row on either side of dw -> dw"""
    lib = _lib.load()

    def ptr(t):
        return t[0].data_ptr() + 4 * t[1] if isinstance(t, tuple) else t.data_ptr()

    ws = filled(dev, (max(BB.wgrad_ws_floats(rows, O, I), 4),), NAN)
    out = filled(dev, (O + 2, I), SENTINEL)
    _lib.check(lib.aaclip_gemm_wgrad(ptr(dz), ldz, ptr(u), ldu, out[1].data_ptr(), rows, O, I, ws.data_ptr(),
                                     ws.numel() * 4, stream(dev)), "gemm_wgrad")
    torch.cuda.synchronize()
    assert bool((out[0] == SENTINEL).all()) and bool((out[O + 1] == SENTINEL).all()), "a row beside dw was written"
    return out[1:O + 1].clone()


@pytest.mark.parametrize("rows,O,I", BB.WGRAD_CASES)
def test_wgrad_per_element(dev, rows, O, I):
    dz, u, want, mag = BB.wgrad_case(rows, O, I)
    dzd, ud = dz.to(dev), u.to(dev)
    got = wgrad(dev, dzd, O, ud, I, rows, O, I)
    assert torch.isfinite(got).all()                        # nothing of the NaN workspace is read before it is written
    err = (got.double().cpu() - want).abs()
    bound = BB.wgrad_bound(rows, mag)
    r = float((err / bound).max())
    print("wgrad", rows, O, I, "chunks", BB.wgrad_chunking(rows), "largest |err| / bound:", r)
    PARITY_ERRORS[f"backward_blocks.wgrad.rows{rows}.{O}x{I}"] = r
    assert bool((err <= bound).all()), r
    assert torch.equal(got, wgrad(dev, dzd, O, ud, I, rows, O, I))          # two calls, equal bits
    assert torch.equal(got, engine.gemm_wgrad(dzd, ud))                     # and the wrapper's call is this one


@pytest.mark.parametrize("rows,O,I", BB.WGRAD_EXACT_CASES)
def test_wgrad_exact_integers(dev, rows, O, I):
    """Small-integer operands are exact in any summation order: any wrong lane, tile, chunk or row mapping shows bit
    for bit."""
    dz, u, want = BB.wgrad_exact_case(rows, O, I)
    got = wgrad(dev, dz.to(dev), O, u.to(dev), I, rows, O, I)
    assert torch.equal(got.double().cpu(), want)


@pytest.mark.parametrize("rows,O,I", BB.WGRAD_STRIDED_CASES)
def test_wgrad_strided_operands(dev, rows, O, I):
    """ldz = O + 4, ldu = I + 132: the operands are column windows of larger buffers whose other columns, and whose rows
    past `rows`, hold NaN.  Bit-identical to the contiguous call."""
    dz, u, _, _ = BB.wgrad_case(rows, O, I)
    ldz, ldu = O + BB.WGRAD_PAD_Z, I + BB.WGRAD_PAD_U
    zb, ub = filled(dev, (rows + 3, ldz), NAN), filled(dev, (rows + 3, ldu), NAN)
    zb[:rows, BB.WGRAD_OFF_Z:BB.WGRAD_OFF_Z + O] = dz.to(dev)
    ub[:rows, BB.WGRAD_OFF_U:BB.WGRAD_OFF_U + I] = u.to(dev)
    got = wgrad(dev, (zb, BB.WGRAD_OFF_Z), ldz, (ub, BB.WGRAD_OFF_U), ldu, rows, O, I)
    assert torch.isfinite(got).all()
    assert torch.equal(got, wgrad(dev, dz.to(dev), O, u.to(dev), I, rows, O, I))


# ---------------------------------------------------------------------------------------------- LayerNorm backward
def ln_backward(dev, x, w, dy, dr, rows, alias=None):
    """aaclip_layernorm_backward on buffers with tail rows (NaN behind the inputs, a sentinel behind a separate output)
    -> d_x [rows, D].  alias: None, "d_y" or "d_resid" = the output is that input's buffer."""
    lib = _lib.load()
    D = x.shape[1]
    xb, yb = with_tail(x, dev), with_tail(dy, dev)
    rb = with_tail(dr, dev) if dr is not None else None
    out, fill = {None: (filled(dev, (rows + BB.TAIL_ROWS, D), SENTINEL), SENTINEL), "d_y": (yb, NAN),
                 "d_resid": (rb, NAN)}[alias]
    _lib.check(lib.aaclip_layernorm_backward(xb.data_ptr(), w.to(dev).data_ptr(), yb.data_ptr(),
                                             None if rb is None else rb.data_ptr(), out.data_ptr(), rows, D,
                                             BB.LN_EPS, stream(dev)), "layernorm_backward")
    torch.cuda.synchronize()
    assert tail_untouched(out, rows, fill), "a row past `rows` was written"
    return out[:rows].clone()


@pytest.mark.parametrize("D,rows,kind", BB.LN_CASES)
def test_layernorm_backward_per_element(dev, D, rows, kind):
    (x, w, b, dy, dr), want = BB.ln_case(D, rows, kind)
    plain = ln_backward(dev, x, w, dy, None, rows)
    resid = ln_backward(dev, x, w, dy, dr, rows)
    check_bound(f"layernorm.D{D}.rows{rows}.{kind}", plain, *want["plain"], BB.LN_K)
    check_bound(f"layernorm.D{D}.rows{rows}.{kind}.resid", resid, *want["resid"], BB.LN_K)
    # the aliasing of block_backward_body and tap_head_backward: the same bits
    assert torch.equal(ln_backward(dev, x, w, dy, None, rows, alias="d_y"), plain)
    assert torch.equal(ln_backward(dev, x, w, dy, dr, rows, alias="d_y"), resid)
    assert torch.equal(ln_backward(dev, x, w, dy, dr, rows, alias="d_resid"), resid)
    assert torch.equal(engine.layernorm_backward(x.to(dev), w.to(dev), dy.to(dev), dr.to(dev)), resid)


# ---------------------------------------------------------------------------------------------- adapter-mix backward
def mix_backward(dev, u, z, dy, mix, rows, alias=False):
    """aaclip_adapter_mix_backward -> (d_z, d_u); alias: d_z overwrites z and d_u overwrites d_y, as in
    block_backward_body"""
    lib = _lib.load()
    D = u.shape[1]
    ub, zb, yb = with_tail(u, dev), with_tail(z, dev), with_tail(dy, dev)
    if alias:
        oz, ou, fill = zb, yb, NAN
    else:
        oz, ou, fill = filled(dev, zb.shape, SENTINEL), filled(dev, zb.shape, SENTINEL), SENTINEL
    _lib.check(lib.aaclip_adapter_mix_backward(ub.data_ptr(), zb.data_ptr(), yb.data_ptr(), oz.data_ptr(), ou.data_ptr(),
                                               rows, D, mix, stream(dev)), "adapter_mix_backward")
    torch.cuda.synchronize()
    assert tail_untouched(oz, rows, fill) and tail_untouched(ou, rows, fill), "a row past `rows` was written"
    return oz[:rows].clone(), ou[:rows].clone()


def run_mix_case(dev, D, rows, kind, mix):
    (u, z, dy), want, terms = BB.mix_case(D, rows, kind, mix)
    d_z, d_u = mix_backward(dev, u, z, dy, mix, rows)
    key = f"adapter_mix.D{D}.rows{rows}.{kind}.mix{mix}"
    check_bound(key + ".d_z", d_z, want[0], terms[0], BB.MIX_K)
    check_bound(key + ".d_u", d_u, want[1], terms[1], BB.MIX_K)
    a_z, a_u = mix_backward(dev, u, z, dy, mix, rows, alias=True)
    assert torch.equal(a_z, d_z) and torch.equal(a_u, d_u)
    e_z, e_u = engine.adapter_mix_backward(u.to(dev), z.to(dev), dy.to(dev), mix)
    assert torch.equal(e_z, d_z) and torch.equal(e_u, d_u)
    return d_z, want[0]


@pytest.mark.parametrize("D,rows,kind,mix", BB.MIX_CASES)
def test_adapter_mix_backward_per_element(dev, D, rows, kind, mix):
    run_mix_case(dev, D, rows, kind, mix)


@pytest.mark.parametrize("D,rows,kind,mix", BB.MIX_ZERO_CASES)
def test_adapter_mix_backward_at_exact_zeros(dev, D, rows, kind, mix):
    """z = +0.0 and z = -0.0 take LeakyReLU's slope 0.01, as torch's leaky_relu backward does: a slope of 1 there is a
    hundred times the reference and far outside the bound (tests/test_backward_blocks_cpu.py shows that it is)."""
    d_z, want = run_mix_case(dev, D, rows, kind, mix)
    at = BB.mix_case(D, rows, kind, mix)[0][1] == 0
    assert rel(d_z.cpu()[at], want[at]) <= 1e-4


# ---------------------------------------------------------------------------------------------- the heads
def tap_head_backward(dev, t, B, L, act):
    """aaclip_tap_head_backward, seg and det part and d_x, with a NaN-filled workspace and sentinel rows behind the three
    outputs -> {d_x, d_proj_w, d_det_w}"""
    lib = _lib.load()
    D, E = t["x"].shape[1], t["proj_w"].shape[0]
    d = {k: v.to(dev).contiguous() for k, v in t.items()}
    pwt, dwt = d["proj_w"].t().contiguous(), d["det_w"].t().contiguous()
    ws = filled(dev, (lib.aaclip_tap_head_backward_workspace_bytes(B, L, D, E) // 4 + 4,), NAN)
    d_x = filled(dev, (B * L + BB.TAIL_ROWS, D), SENTINEL)
    d_pw, d_dw = filled(dev, (E + 1, D), SENTINEL), filled(dev, (E + 1, D), SENTINEL)
    _lib.check(lib.aaclip_tap_head_backward(d["x"].data_ptr(), d["ln_w"].data_ptr(), d["ln_b"].data_ptr(),
                                            d["proj_w"].data_ptr(), pwt.data_ptr(), act, d["d_seg"].data_ptr(),
                                            d["det_w"].data_ptr(), dwt.data_ptr(), d["d_det"].data_ptr(), d_x.data_ptr(),
                                            d_pw.data_ptr(), d_dw.data_ptr(), B, L, D, E, ws.data_ptr(), ws.numel() * 4,
                                            stream(dev)), "tap_head_backward")
    torch.cuda.synchronize()
    assert tail_untouched(d_x, B * L, SENTINEL) and tail_untouched(d_pw, E, SENTINEL) and tail_untouched(d_dw, E, SENTINEL)
    return {"d_x": d_x[:B * L].clone(), "d_proj_w": d_pw[:E].clone(), "d_det_w": d_dw[:E].clone()}


def run_head_case(dev, name):
    B, L, D, E, act, zero_row = BB.ALL_HEAD_CASES[name]
    t, want, terms = BB.head_case(name)
    got = tap_head_backward(dev, t, B, L, act)
    for k in BB.HEAD_OUTPUTS:
        check_bound(f"tap_head.{name}.{k}", got[k], want[k], terms[k], BB.HEAD_K)
    assert not got["d_x"].reshape(B, L, D)[:, 0, :].any()                      # CLS rows: exact zeros
    return got, want


@pytest.mark.parametrize("name", list(BB.HEAD_CASES))
def test_tap_head_backward_per_element(dev, name):
    run_head_case(dev, name)


@pytest.mark.parametrize("name", list(BB.HEAD_ZERO_CASES))
def test_tap_head_backward_at_exact_zeros(dev, name):
    """One all-zero row of proj_w and of det_w: that feature's pre-activation is exactly 0 in every row, and that row of
    the weight gradients differs by a factor of 100 between LeakyReLU slopes 0.01 (torch, the reference) and 1."""
    B, L, D, E, act, zero_row = BB.HEAD_ZERO_CASES[name]
    got, want = run_head_case(dev, name)
    for k in ("d_proj_w", "d_det_w"):
        if act == BB.LEAKY:
            assert rel(got[k][zero_row], want[k][zero_row]) <= 1e-4, k
        else:
            assert not got[k][zero_row].any() and not want[k][zero_row].any()  # ReLU: slope 0 at 0


def row_head_backward(dev, t, name):
    """aaclip_row_head_backward with a NaN-filled workspace and sentinel rows behind both outputs -> {d_x, d_proj_w}"""
    lib = _lib.load()
    n, T, D, E, act, zero_row, eot = BB.ROW_HEAD_ZERO_CASES[name]
    d = {k: v.to(dev).contiguous() for k, v in t.items()}
    pwt = d["proj_w"].t().contiguous()
    ws = filled(dev, (lib.aaclip_text_backward_workspace_bytes(n * T, D, 0) // 4 + 4,), NAN)
    d_x, d_w = filled(dev, (n * T + BB.TAIL_ROWS, D), SENTINEL), filled(dev, (E + 1, D), SENTINEL)
    _lib.check(lib.aaclip_row_head_backward(d["x"].data_ptr(), d["tokens"].data_ptr(), d["ln_w"].data_ptr(),
                                            d["ln_b"].data_ptr(), d["proj_w"].data_ptr(), pwt.data_ptr(), act,
                                            d["d_out"].data_ptr(), d_x.data_ptr(), d_w.data_ptr(), n, T, D, E, 0,
                                            ws.data_ptr(), ws.numel() * 4, stream(dev)), "row_head_backward")
    torch.cuda.synchronize()
    assert tail_untouched(d_x, n * T, SENTINEL) and tail_untouched(d_w, E, SENTINEL)
    return {"d_x": d_x[:n * T].clone(), "d_proj_w": d_w[:E].clone()}


@pytest.mark.parametrize("name", list(BB.ROW_HEAD_ZERO_CASES))
def test_row_head_backward_at_exact_zeros(dev, name):
    """The same for the element-wise act' of the row head (n E / 4 = 960: no multiple of the 256 threads of a workgroup;
    256: exactly one)."""
    zero_row = BB.ROW_HEAD_ZERO_CASES[name][5]
    t, want, terms = BB.row_head_case(name)
    got = row_head_backward(dev, t, name)
    for k in BB.ROW_HEAD_OUTPUTS:
        check_bound(f"row_head.{name}.{k}", got[k], want[k], terms[k], BB.HEAD_K)
    assert rel(got["d_proj_w"][zero_row], want["d_proj_w"][zero_row]) <= 1e-4


# ---------------------------------------------------------------------------------------------- short attention backward
@pytest.mark.parametrize("L,causal,peak", BB.ATTN_CASES)
def test_attention_backward_segments(dev, L, causal, peak):
    """The short kernel and, as a second implementation of the same function, the tiled kernels at the same length: each
    against fp64, never against each other."""
    qkv, d_ctx, want = BB.attention_case(L, causal, peak)
    bar = BB.attention_segment_bar(L, peak)
    for which, long_rows in (("short", None), ("tiled", True)):
        got = engine.attention_backward(qkv.to(dev), d_ctx.to(dev), BB.ATTN_B, L, BB.ATTN_H, causal, long_rows=long_rows)
        assert torch.isfinite(got).all()
        whole, seg = rel(got, want), BB.segment_error(got, want, L)
        key = f"attention.{which}.{'causal' if causal else 'full'}.L{L}" + ("" if peak is None else ".peaked")
        print(key, "whole", whole, "segment", seg, "of", bar)
        PARITY_ERRORS["backward_blocks." + key] = {"whole": whole, "segment": seg}
        assert whole <= BB.ATTN_WHOLE_BAR, (which, whole)
        assert seg <= bar, (which, seg, bar)
        if causal and which == "short":                                        # the first row attends to itself alone
            D = 64 * BB.ATTN_H
            assert not got.reshape(BB.ATTN_B, L, 3 * D)[:, 0, :D].any()
