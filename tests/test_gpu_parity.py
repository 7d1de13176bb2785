"""GPU parity tests: every call goes through the C ABI of libaaclip_hip.so and is
compared with the CPU oracle (oracle/aaclip_oracle.py, pinned to the reference)
and with the committed golden vectors produced by the reference itself.

Tolerances (written where used):
  * fp32 MFMA path ('fp32'): 2e-4 abs + 1e-3 rel on tower outputs.
  * fp16 MFMA path ('fp16'): BASELINE.json north_star -- 1e-3 abs + 1e-2 rel --
    applied to the API outputs: unit-norm seg tokens, det token, text
    embeddings (as the cosine they feed), and anomaly maps.
  * bf16: 8-bit mantissa; offered, not the parity path: 1e-2 abs + 5e-2 rel.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from aaclip_hip import _lib, engine, synth
from aaclip_hip._lib import BF16, F16, F16X2, F32
from conftest import GOLDEN, PARITY_ERRORS
from oracle import aaclip_oracle as O

pytestmark = pytest.mark.gpu
T = torch.from_numpy
TDT = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}
NAME = {F32: "fp32", F16: "fp16", BF16: "bf16", F16X2: "fp16x2"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def assert_close(a, b, atol, rtol, what=""):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.isfinite(a).all(), f"{what}: non-finite output"
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = err > tol
    assert not bad.any(), (f"{what}: {int(bad.sum())}/{bad.numel()} outside {atol}+{rtol}*|ref|; "
                           f"max err {err.max().item():.3e} at ref {b.flatten()[err.argmax()].item():.3e}")


# fp16x2 (fp16 main term + e4m3 correction terms): asserted 2x tighter than the north star on these small models
TOL = {F32: (2e-4, 1e-3), F16: (1e-3, 1e-2), BF16: (1e-2, 5e-2), F16X2: (5e-4, 5e-3)}


# ----------------------------------------------------------------------------
# kernels
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("D", [256, 768, 1024])
@pytest.mark.parametrize("code", [F32, F16, BF16])
def test_layernorm(dev, D, code):
    lib = _lib.load()
    x = synth.randn("t.ln.x", (37, D), 3.0, 1, mean=0.7)
    w, b = synth.randn("t.ln.w", (D,), 0.2, 1, 1.0), synth.randn("t.ln.b", (D,), 0.2, 1)
    out = torch.empty(37, D, dtype=TDT[code], device=dev)
    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    _lib.check(lib.aaclip_layernorm(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), code, 37, D, 1e-5,
                                    stream(dev)))
    ref = O.layer_norm(x.double(), w.double(), b.double())
    atol = {F32: 2e-6, F16: 2e-3, BF16: 2e-2}[code]
    assert_close(out.float(), ref, atol, 1e-5 if code == F32 else 1e-2, f"layernorm {D}")


def _gemm(lib, dev, code, epi, A, W, bias, out, act=0, scale_cols=0, scale=1.0):
    M, K = A.shape
    N = W.shape[0]
    _lib.check(lib.aaclip_gemm(code, epi, A.data_ptr(), K, W.data_ptr(), None if bias is None else bias.data_ptr(),
                               out.data_ptr(), out.shape[1], M, N, K, act, scale_cols, scale, stream(dev)), "gemm")


@pytest.mark.parametrize("code", [F32, F16, BF16])
def test_gemm_exact_integers(dev, code):
    """Small-integer operands are exact in every dtype: catches any wrong lane /
    fragment / swizzle mapping bit-for-bit (asymmetric A and W, ragged M)."""
    lib = _lib.load()
    M, N, K = 200, 256, 192
    g = torch.Generator().manual_seed(5)
    A = torch.randint(-3, 4, (M, K), generator=g).float()
    W = torch.randint(-2, 3, (N, K), generator=g).float()
    A[:, 0] += torch.arange(M).float() % 5   # asymmetric in both dims
    W[:, 1] += torch.arange(N).float() % 3
    ref = A.double() @ W.double().t()
    out = torch.zeros(M, N, dtype=torch.float32, device=dev)
    _gemm(lib, dev, code, _lib.EPI_ACT_F32, A.to(dev, TDT[code]).contiguous(), W.to(dev, TDT[code]).contiguous(),
          None, out)
    assert torch.equal(out.cpu().double(), ref)


@pytest.mark.parametrize("code", [F32, F16, BF16])
@pytest.mark.parametrize("shape", [(1370, 1024, 1024), (300, 128, 64), (77, 768, 3072), (129, 384, 640),
                                   (4100, 256, 192),     # large M, odd K/64: the fallback 256-tile kernel
                                   (5000, 768, 1024)])   # large M, ragged last tile: the default 256-tile kernel
def test_gemm_epilogues(dev, code, shape):
    lib = _lib.load()
    M, N, K = shape
    A = synth.randn("t.g.a", (M, K), 1.0, 2).to(TDT[code])
    W = synth.randn("t.g.w", (N, K), K ** -0.5, 2).to(TDT[code])
    bias = synth.randn("t.g.b", (N,), 0.5, 2)
    Ad, Wd, bd = A.to(dev), W.to(dev), bias.to(dev)
    acc = A.double() @ W.double().t()
    et = {F32: 1e-5, F16: 1.5e-3, BF16: 1.2e-2}[code]   # output rounding to the compute dtype
    # bias (+ q scaling of the first 64 columns)
    out = torch.empty(M, N, dtype=TDT[code], device=dev)
    _gemm(lib, dev, code, _lib.EPI_BIAS, Ad, Wd, bd, out, scale_cols=64, scale=0.125)
    ref = acc + bias.double()
    ref[:, :64] *= 0.125
    assert_close(out.float(), ref, et, et, "bias")
    # bias + exact gelu
    _gemm(lib, dev, code, _lib.EPI_BIAS_GELU, Ad, Wd, bd, out)
    assert_close(out.float(), O.gelu_erf(acc + bias.double()), et, et, "gelu")
    # bias + residual in place (fp32)
    x0 = synth.randn("t.g.x", (M, N), 2.0, 2)
    xd = x0.to(dev)
    _gemm(lib, dev, code, _lib.EPI_BIAS_RESID, Ad, Wd, bd, xd)
    assert_close(xd, x0.double() + acc + bias.double(), 2e-5, 1e-5, "resid")
    # leaky fp32
    o32 = torch.empty(M, N, dtype=torch.float32, device=dev)
    _gemm(lib, dev, code, _lib.EPI_ACT_F32, Ad, Wd, None, o32, act=1)
    assert_close(o32, O.leaky_relu(acc), 2e-5, 1e-5, "leaky")


def test_gemm_fp32_tile_forms_are_bit_identical(dev):
    """The exact-fp32 GEMM has a 128 x 128-tile and a 64 x 64-tile form (small grids: csrc/gemm.hip); every output element
    sums its k terms in the same order in both, so the same columns computed inside a wide product (128-tile form: >= 128
    tiles) and alone (64-tile form) must agree bit for bit."""
    lib = _lib.load()
    M, K, NW = 200, 272, 8192
    A = synth.randn("t.g32.a", (M, K), 1.0, 3).to(dev)
    W = synth.randn("t.g32.w", (NW, K), K ** -0.5, 4).to(dev)
    bias = synth.randn("t.g32.b", (NW,), 0.5, 5).to(dev)
    wide = torch.empty(M, NW, dtype=torch.float32, device=dev)
    _gemm(lib, dev, F32, _lib.EPI_BIAS_GELU, A, W, bias, wide)
    for n0, n in ((0, 128), (1024, 384)):
        alone = torch.empty(M, n, dtype=torch.float32, device=dev)
        _gemm(lib, dev, F32, _lib.EPI_BIAS_GELU, A, W[n0:n0 + n].contiguous(), bias[n0:n0 + n].contiguous(), alone)
        assert torch.equal(alone, wide[:, n0:n0 + n]), (n0, n)


def _attn_ref(qkv, B, L, H, causal):
    D = H * 64
    q, k, v = qkv.double().view(B, L, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2)
    if causal:
        s = s + O.causal_mask(L, torch.float64)
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * L, D)


@pytest.mark.parametrize("code", [F32, F16, BF16])
@pytest.mark.parametrize("cfg", [(2, 1370, 2, 0), (3, 77, 4, 1), (1, 50, 1, 0), (2, 130, 2, 1), (1, 64, 1, 0),
                                 (1, 129, 1, 1), (5, 1, 2, 0), (26, 3, 4, 0), (7, 2, 1, 1)])
def test_attention(dev, code, cfg):
    lib = _lib.load()
    B, L, H, causal = cfg
    D = H * 64
    qkv = synth.randn("t.attn", (B * L, 3 * D), 1.0, 3)
    qkv[:, :D] *= 0.6            # q already carries the 1/8 scale in the real path; keep logits O(5)
    qkv = qkv.to(TDT[code])
    ctx = torch.full((B * L, D), float("nan"), dtype=TDT[code], device=dev)
    qd = qkv.to(dev)
    _lib.check(lib.aaclip_attention(code, qd.data_ptr(), ctx.data_ptr(), B, L, H, causal, stream(dev)), "attention")
    ref = _attn_ref(qkv.float(), B, L, H, causal)
    tol = {F32: (2e-5, 1e-5), F16: (3e-3, 1e-2), BF16: (2.5e-2, 3e-2)}[code]
    assert_close(ctx.float(), ref, tol[0], tol[1], f"attention {cfg}")


def test_attention_online_softmax_rescale(dev):
    """Force the running max to jump at a late key tile (guide rule 26): one key
    with a huge logit in the last tile; rows must still sum correctly."""
    lib = _lib.load()
    B, L, H = 1, 300, 1
    qkv = synth.randn("t.attn.spike", (L, 192), 0.5, 4)
    qkv[:, 0] = 1.0           # q[:,0] = 1
    qkv[290, 64] = 40.0       # k[290,0] = 40 -> logit +40 on every row, appears in tile 4
    for code in (F32, F16):
        q = qkv.to(TDT[code])
        ctx = torch.empty(L, 64, dtype=TDT[code], device=dev)
        qd = q.to(dev)
        _lib.check(lib.aaclip_attention(code, qd.data_ptr(), ctx.data_ptr(), B, L, H, 0, stream(dev)))
        ref = _attn_ref(q.float(), B, L, H, 0)
        assert_close(ctx.float(), ref, 3e-3 if code == F16 else 2e-5, 1e-2 if code == F16 else 1e-5, "spike")


@pytest.mark.parametrize("code", [F16, BF16])
@pytest.mark.parametrize("cfg", [(2, 1370, 2, 0), (1, 640, 3, 1), (3, 77, 4, 1), (1, 50, 1, 0)])
def test_attention_log2q_variant(dev, code, cfg):
    """aaclip_attention_log2q: the kernel variant aaclip_block runs (q already in log2 units, one v_exp_f32 per score)
    against fp64 softmax of (q . k) * ln 2."""
    lib = _lib.load()
    B, L, H, causal = cfg
    D = H * 64
    qkv = synth.randn("t.attn.l2", (B * L, 3 * D), 1.0, 5)
    qkv[:, :D] *= 0.6 * 1.4426950408889634
    qkv = qkv.to(TDT[code])
    ctx = torch.full((B * L, D), float("nan"), dtype=TDT[code], device=dev)
    qd = qkv.to(dev)
    _lib.check(lib.aaclip_attention_log2q(code, qd.data_ptr(), ctx.data_ptr(), B, L, H, causal, stream(dev)))
    f = qkv.float().clone()
    f[:, :D] *= 0.6931471805599453
    ref = _attn_ref(f, B, L, H, causal)
    tol = (3e-3, 1e-2) if code == F16 else (2.5e-2, 3e-2)
    assert_close(ctx.float(), ref, tol[0], tol[1], f"attention log2q {cfg}")
    assert lib.aaclip_attention_log2q(F32, qd.data_ptr(), ctx.data_ptr(), B, L, H, causal, stream(dev)) < 0


@pytest.mark.parametrize("causal", [0, 1])
def test_attention_long_sequence_rebase_paths(dev, causal):
    """The long-sequence kernel (L >= 512) exponentiates against the reference point a row already has and only
    re-bases when a tile breaks the 16-bit bound of its probabilities (attention.hip, `tile`): force every path --
    tile 0 (always exact), quiet tiles (fast), a +40 logit in tile 5 (partial sums beyond the bound -> exact redo), a
    +150 logit in tile 9 (2^216: the fast pass overflows fp32 to inf -> exact redo), rows with NEGATIVE scores only
    in tile 0 (m starts below 0), and the ragged last tile."""
    lib = _lib.load()
    B, L, H = 2, 700, 2
    D = 64 * H
    qkv = synth.randn("t.attn.long", (B * L, 3 * D), 0.5, 8)
    qkv[:, 0] = 1.0                     # q[:, 0] = 1 in head 0
    qkv[:64, D] = -6.0                  # keys 0..63 of image 0 (tile 0): logits about -6 for every row
    qkv[5 * 64 + 7, D] = 40.0           # k[327, 0]: logit +40 (tile 5)
    qkv[9 * 64 + 30, D] = 150.0         # k[606, 0]: logit +150 (tile 9)
    qkv[L + 650, D + 64] = 90.0         # image 1, head 1, tile 10 -- with q[:, 64] = 1
    qkv[L:, 64] = 1.0
    for code in (F16, BF16):
        q = qkv.to(TDT[code])
        ctx = torch.full((B * L, D), float("nan"), dtype=TDT[code], device=dev)
        qd = q.to(dev)
        _lib.check(lib.aaclip_attention(code, qd.data_ptr(), ctx.data_ptr(), B, L, H, causal, stream(dev)))
        ref = _attn_ref(q.float(), B, L, H, causal)
        tol = (3e-3, 1e-2) if code == F16 else (2.5e-2, 3e-2)
        assert_close(ctx.float(), ref, tol[0], tol[1], f"long-sequence re-base paths causal={causal} {NAME[code]}")


def test_adapter_mix(dev):
    lib = _lib.load()
    x = synth.randn("t.mix.x", (41, 1024), 2.0, 5)
    a = synth.randn("t.mix.a", (41, 1024), 0.3, 5)
    xd, ad = x.to(dev), a.to(dev)
    _lib.check(lib.aaclip_adapter_mix(xd.data_ptr(), ad.data_ptr(), 41, 1024, 0.1, stream(dev)))
    ref = 0.1 * (a.double() * x.double().norm(dim=-1, keepdim=True) / a.double().norm(dim=-1, keepdim=True)) + 0.9 * x.double()
    assert_close(xd, ref, 1e-5, 1e-5, "mix")


# ----------------------------------------------------------------------------
# models
# ----------------------------------------------------------------------------
def build_tiny(dev, precision):
    from model.model import CLIP
    from model.adapter import AdaptedCLIP
    cfg = synth.tiny_cfg()
    sd = synth.synth_clip_state_dict(cfg, seed=7)
    clip = CLIP(cfg.embed_dim,
                dict(image_size=cfg.image_size, layers=cfg.vision.layers, width=cfg.vision.width,
                     patch_size=cfg.patch_size),
                dict(context_length=77, vocab_size=cfg.vocab_size, width=cfg.text.width, heads=cfg.text.heads,
                     layers=cfg.text.layers), precision=precision)
    clip.load_state_dict(sd, strict=True)
    ia = synth.synth_image_adapter_state_dict(cfg, until=2, levels=2, seed=7)
    ta = synth.synth_text_adapter_state_dict(cfg, until=1, seed=7)
    model = AdaptedCLIP(clip, text_adapt_until=1, image_adapt_until=2, levels=[2, 3], relu=False)
    model.image_adapter.load_state_dict(ia, strict=True)
    model.text_adapter.load_state_dict(ta, strict=True)
    return cfg, sd, ia, ta, clip.to(dev).eval(), model.to(dev).eval()


@pytest.mark.parametrize("code", [F32, F16X2, F16, BF16])
def test_tiny_clip_vs_reference_golden(dev, golden_tiny, code):
    """CLIP.encode_image / encode_text against outputs of the reference itself."""
    cfg, sd, ia, ta, clip, model = build_tiny(dev, NAME[code])
    img = synth.synth_images(3, cfg.image_size, seed=7).to(dev)
    atol, rtol = TOL[code]
    with torch.no_grad():
        pooled, taps = clip.encode_image(img, [1, 3])
        txt = clip.encode_text(T(golden_tiny["tiny.tokens"]).to(dev))
    # residual stream values are O(1..5): the north-star tolerance is relative there
    s = 4 if code in (F16, BF16) else 1
    assert_close(taps[0], T(golden_tiny["tiny.tap1"]), s * atol, rtol, "tap1")
    assert_close(taps[1], T(golden_tiny["tiny.tap3"]), s * atol, rtol, "tap3")
    assert_close(pooled, T(golden_tiny["tiny.pooled"]), s * atol, rtol, "pooled")
    assert_close(txt, T(golden_tiny["tiny.text"]), s * atol, rtol, "text")


def test_tiny_fp16_exact_weights_take_the_three_plane_form(dev):
    """fp16x2 with CLIP weights that are exact in fp16: the engine passes those matrices without their lo plane
    (aaclip_block_weights.exact16) and the small-batch split kernel skips the weight-lo correction tile -- same
    function of the rounded weights, checked against the fp64 oracle on the rounded weights."""
    from aaclip_hip import engine as E
    cfg, sd, ia, ta, clip, model = build_tiny(dev, "fp16x2")
    sdh = {k: (v.half().float() if v.is_floating_point() else v) for k, v in sd.items()}
    clip.load_state_dict(sdh, strict=True)
    blk = clip.visual.transformer.resblocks[0]
    w, refs = E.pack_block(blk, F16X2, None)
    assert w.exact16 == 15                                  # qkv, out, fc, proj all exact and K % 256 == 0
    assert E.CACHE.get(blk.mlp.c_fc.weight, F16X2, "plain+exact").shape[1] == 3 * blk.mlp.c_fc.weight.shape[1]
    img = synth.synth_images(3, cfg.image_size, seed=7)
    with torch.no_grad():
        pooled, taps = clip.encode_image(img.to(dev), [1, 3])
    opooled, otaps = O.encode_image(img, sdh, cfg.vision.heads, [1, 3], dtype=torch.float64)
    assert_close(taps[1], otaps[1], 5e-4, 5e-3, "tap3, fp16-exact weights")
    assert_close(pooled, opooled, 5e-4, 5e-3, "pooled, fp16-exact weights")


@pytest.mark.parametrize("code", [F32, F16X2, F16, BF16])
def test_tiny_adapted_vs_oracle(dev, code):
    cfg, sd, ia, ta, clip, model = build_tiny(dev, NAME[code])
    img = synth.synth_images(3, cfg.image_size, seed=7)
    tok = torch.zeros(2, 77, dtype=torch.int32)
    tok[0, :5] = torch.tensor([49406, 320, 1125, 539, 49407])
    tok[1, :3] = torch.tensor([49406, 13568, 49407])
    atol, rtol = TOL[code]
    with torch.no_grad():
        seg, det, iqm = model(img.to(dev))
        txt = model.encode_text(tok.to(dev))
    assert iqm is None and len(seg) == 2
    oseg, odet = O.adapted_visual_forward(img, sd, ia, cfg.vision.heads, image_adapt_until=2, levels=(2, 3),
                                          dtype=torch.float64)
    otxt = O.adapted_encode_text(tok, sd, ta, cfg.text.heads, text_adapt_until=1, dtype=torch.float64)
    for i in range(2):
        assert_close(seg[i], oseg[i], atol, rtol, f"seg{i}")
    assert_close(det, odet, atol, rtol, "det")
    assert_close(txt, otxt, 4 * atol if code in (F16, BF16) else atol, rtol, "adapted text")


def test_lnd_block_api(dev):
    """resblocks[i](x_lnd, attn_mask=...) keeps the reference's LND calling convention."""
    cfg, sd, ia, ta, clip, model = build_tiny(dev, "fp32")
    x = synth.randn("t.lnd", (26, 2, 256), 1.0, 9)
    y, attn = clip.visual.transformer.resblocks[0](x.to(dev), attn_mask=None)
    ref = O.resblock(x.permute(1, 0, 2).double(), {k: v.double() for k, v in sd.items()},
                     "visual.transformer.resblocks.0.", 4, None).permute(1, 0, 2)
    assert attn is None
    assert_close(y, ref, 2e-4, 1e-3, "lnd block")
    t = synth.randn("t.lnd.t", (77, 2, 256), 1.0, 9)
    y, _ = clip.transformer.resblocks[1](t.to(dev), attn_mask=clip.attn_mask)
    ref = O.resblock(t.permute(1, 0, 2).double(), {k: v.double() for k, v in sd.items()},
                     "transformer.resblocks.1.", 4, O.causal_mask(77, torch.float64)).permute(1, 0, 2)
    assert_close(y, ref, 2e-4, 1e-3, "lnd causal block")
    # ln_post is callable on its own like the reference's modules (train.py:79-81)
    z = clip.visual.ln_post(x.to(dev))
    assert_close(z, O.layer_norm(x.double(), sd["visual.ln_post.weight"].double(), sd["visual.ln_post.bias"].double()),
                 1e-5, 1e-5, "ln_post")


# ----------------------------------------------------------------------------
# anomaly map
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("domain", ["Industrial", "Medical"])
def test_similarity_maps(dev, golden_tiny, domain):
    import forward_utils as FU
    pf, tf = T(golden_tiny["map.pf"]), T(golden_tiny["map.tf"])
    # train-mode: against the reference's own output
    out = FU.calculate_similarity_map(pf.to(dev), tf.to(dev), 70, test=False)
    assert_close(out, T(golden_tiny["map.train"]), 1e-5, 1e-5, "train map")
    # test-mode single level: oracle (blur is parity-unpinned, see oracle header)
    out = FU.calculate_similarity_map(pf.to(dev), tf.to(dev), 70, test=True, domain=domain)
    assert out.shape == (2, 1, 70, 70)
    assert_close(out, O.similarity_map(pf, tf, 70, test=True, domain=domain), 1e-3, 1e-4, "test map")
    # ksize=1 skips the blur: this piece IS pinned by the reference (pre-blur map + F.interpolate)
    raw = engine.anomaly_map([pf.to(dev)], tf.to(dev), 70, 1, 1.0)
    assert_close(raw.unsqueeze(1), T(golden_tiny["map.pre_blur_up"]), 1e-4, 1e-5, "pre-blur upsample")


def test_anomaly_map_full_size_levels(dev):
    import forward_utils as FU
    segs = [torch.nn.functional.normalize(synth.randn(f"t.am.{i}", (3, 1369, 768), 1.0, 11), dim=-1) for i in range(4)]
    anchors = torch.nn.functional.normalize(synth.randn("t.am.t", (768, 2), 1.0, 11), dim=0)
    out = FU.calculate_anomaly_map([s.to(dev) for s in segs], anchors.to(dev), 518, domain="Industrial")
    assert out.shape == (3, 518, 518)
    ref = O.anomaly_map(segs, anchors, 518, "Industrial")
    assert_close(out, ref, 1e-3, 1e-4, "anomaly map")
    # shared anchors == per-image anchors; sum of single-level maps == fused map
    outb = FU.calculate_anomaly_map([s.to(dev) for s in segs], anchors.unsqueeze(0).repeat(3, 1, 1).to(dev), 518,
                                    domain="Industrial")
    assert torch.equal(out, outb)
    parts = sum(FU.calculate_similarity_map(s.to(dev), anchors.to(dev), 518, test=True, domain="Industrial")[:, 0]
                for s in segs)
    assert_close(out, parts, 1e-4, 1e-6, "level sum")


# ----------------------------------------------------------------------------
# full-size ViT-L/14 @518 against the reference's golden vectors
# ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_weights():
    cfg = synth.ClipCfg()
    return (cfg, synth.synth_clip_state_dict(cfg, 111), synth.synth_image_adapter_state_dict(cfg, seed=111),
            synth.synth_text_adapter_state_dict(cfg, seed=111))


def build_full(dev, precision, full_weights):
    from model.clip import create_model
    from model.adapter import AdaptedCLIP
    cfg, sd, ia, ta = full_weights
    clip = create_model("ViT-L-14-336", 518, pretrained=None, precision=precision, force_image_size=518)
    clip.load_state_dict(sd, strict=True)
    model = AdaptedCLIP(clip, relu=False)
    model.image_adapter.load_state_dict(ia, strict=True)
    model.text_adapter.load_state_dict(ta, strict=True)
    return model.to(dev).eval()


def sampled_close(golden, name, t, atol, rtol):
    assert tuple(golden[f"{name}.shape"]) == tuple(t.shape), name
    f = t.detach().reshape(-1).cpu()
    assert_close(f[T(golden[f"{name}.idx"])], T(golden[f"{name}.val"]), atol, rtol, name)


@pytest.mark.parametrize("code", [F32, F16X2, F16])
def test_full_model_vs_reference_golden(dev, golden_full, full_weights, code):
    import forward_utils as FU
    model = build_full(dev, NAME[code], full_weights)
    img = synth.synth_images(2, 518, seed=111).to(dev)
    atol, rtol = TOL[code]
    with torch.no_grad():
        seg, det, _ = model(img)
        tok = T(golden_full["full.text_tokens"]).to(dev)
        txt_a = model.encode_text(tok)
        txt_p = model.encode_text(tok, adapt_text=False)
        anchors = FU.get_adapted_single_class_text_embedding(model, "MVTec", "bottle", dev)
    for i in range(4):
        sampled_close(golden_full, f"full.seg{i}", seg[i], atol, rtol)
        n = seg[i].norm(dim=-1)
        assert float((n - 1).abs().max()) < 1e-5
    assert_close(det, T(golden_full["full.det"]), atol, rtol, "det")
    # text embeddings are only used through their direction (forward_utils.py:155): compare unit vectors
    for name, t in (("full.text_adapted", txt_a), ("full.text_plain", txt_p)):
        g = T(golden_full[name])
        assert_close(torch.nn.functional.normalize(t, dim=-1), torch.nn.functional.normalize(g, dim=-1), atol, rtol, name)
    assert_close(anchors, T(golden_full["full.anchors_bottle"]), atol, rtol, "anchors")
    # maps: pre-blur map of every level on the golden anchors (values O(1..10), x100 amplified cosines)
    ganch = T(golden_full["full.anchors_bottle"]).to(dev)
    for i in range(4):
        raw = engine.anomaly_map([seg[i]], ganch, 37, 1, 1.0)   # S == grid: identity upsample
        # measured on MI355X (tests/test_gpu_configs.py docstring, profiles/r02_parity_errors.json): fp32 path max
        # |err| ~1e-5; fp16 path <= 2.9e-3 per level -- the fp16 tower's rounding noise x50, not the head
        # fp16x2: the north star itself (B = 2: the small-batch kernels; the large-batch ones: test_gpu_configs.py)
        matol = {F32: 1e-4, F16X2: 1e-3}.get(code, 4e-3)
        assert_close(raw, T(golden_full[f"full.map_pre_blur{i}"]), matol, rtol if code != F32 else 1e-3, f"pre-blur map {i}")
    tfb = ganch.unsqueeze(0).repeat(2, 1, 1)
    sampled_close(golden_full, "full.map_train3", FU.calculate_similarity_map(seg[3], tfb, 518, test=False),
                  {F32: 2e-4, F16X2: 5e-4}.get(code, 2e-3), rtol)


def test_full_encode_image_vs_reference_golden(dev, golden_full, full_weights):
    model = build_full(dev, "fp16", full_weights)
    img = synth.synth_images(1, 518, seed=111).to(dev)
    with torch.no_grad():
        pooled, taps = model.clipmodel.encode_image(img, [6, 24])
    assert taps[0].shape == (1, 1370, 1024)
    sampled_close(golden_full, "full.tap6", taps[0], 4e-3, 1e-2)
    sampled_close(golden_full, "full.tap24", taps[1], 4e-3, 1e-2)
    assert_close(pooled, T(golden_full["full.pooled"]), 4e-3, 1e-2, "pooled")


def test_batch_independence_and_determinism(dev, full_weights):
    """Size-independent properties at a larger batch: two runs are bit-identical; image i gives the
    bit-identical result in every batch served by the same kernels (B >= 3: 256-tile GEMMs with ln_2 folded
    into c_fc; B <= 2: 128-tile GEMMs with the ln_2 pass), and the same result within the fp16 tolerance
    across the two regimes (they differ in where ln_2's rounding happens, not in the math)."""
    model = build_full(dev, "fp16", full_weights)
    img = synth.synth_images(5, 518, seed=3).to(dev)
    with torch.no_grad():
        seg_a, det_a, _ = model(img)
        seg_b, det_b, _ = model(img)
        seg_3, det_3, _ = model(img[1:4])
        seg_2, det_2, _ = model(img[2:4])
        seg_1, det_1, _ = model(img[3:4])
    for a, b in zip(seg_a, seg_b):
        assert torch.equal(a, b)
    assert torch.equal(det_a, det_b)
    for a, s in zip(seg_a, seg_3):
        assert torch.equal(a[1:4], s)
    assert torch.equal(det_a[1:4], det_3)
    for a, s in zip(seg_2, seg_1):
        assert torch.equal(a[1:2], s)
    assert torch.equal(det_2[1:2], det_1)
    atol, rtol = TOL[F16]
    for i, (a, s) in enumerate(zip(seg_a, seg_1)):
        assert_close(a[3:4], s, atol, rtol, f"seg{i} across kernel regimes")
    assert_close(det_a[3:4], det_1, atol, rtol, "det across kernel regimes")


def test_ln_fold_matches_ln_pass(dev, full_weights):
    """ln_2 folded into c_fc (aaclip_block_weights.fc_w_fold) against the same block with the ln_2 pass:
    one full-size block on B = 4, both against the fp32 oracle block and against each other."""
    lib = _lib.load()
    cfg, sd, ia, ta = full_weights
    model = build_full(dev, "fp16", full_weights)
    blk = model.image_encoder.transformer.resblocks[3]
    B, L, D = 4, 1370, 1024
    x0 = synth.randn("t.fold.x", (B * L, D), 1.0, 9)
    x0[:, 5] += 3.0          # a column with a large mean: the folded form must cancel it
    outs = []
    for flag in (0, 1 << 17):
        lib.aaclip_set_gemm_variant(flag)
        x = x0.clone().to(dev)
        engine.run_block(x, blk, B, L, 16, F16)
        outs.append(x.cpu())
    lib.aaclip_set_gemm_variant(0)
    ref = O.resblock(x0.view(B, L, D).double(), {k: v.double() for k, v in sd.items()},
                     "visual.transformer.resblocks.3.", 16, None).view(B * L, D)
    assert_close(outs[0], ref, 4e-3, 1e-2, "folded block vs oracle")
    assert_close(outs[1], ref, 4e-3, 1e-2, "block with ln_2 pass vs oracle")
    assert_close(outs[0], outs[1], 4e-3, 1e-2, "folded vs ln_2 pass")


# ----------------------------------------------------------------------------
# metric parity: AUROC of the anomaly map on synthetic masks (no dataset in the container)
# ----------------------------------------------------------------------------
def test_auroc_parity_on_synthetic_masks(dev, full_weights):
    """BASELINE.json: 'patch-anomaly-map AUROC parity'.  Pixel AUROC / AP of the HIP map vs
    the oracle's map against the same synthetic ground-truth masks: |delta| <= 1e-3."""
    import forward_utils as FU
    from sklearn.metrics import roc_auc_score
    cfg, sd, ia, ta = full_weights
    model = build_full(dev, "fp16", full_weights)
    B = 4
    img = synth.synth_images(B, 518, seed=21)
    masks = synth.synth_masks(B, 518, seed=21).numpy()
    tok = torch.zeros(2, 77, dtype=torch.int32)
    tok[0, :4] = torch.tensor([49406, 1125, 539, 49407])
    tok[1, :5] = torch.tensor([49406, 320, 13568, 539, 49407])
    with torch.no_grad():
        seg, det, _ = model(img.to(dev))
        txt = model.encode_text(tok.to(dev))
        anchors = torch.stack([txt[0] / txt[0].norm(), txt[1] / txt[1].norm()], dim=1)
        amap = FU.calculate_anomaly_map(seg, anchors, 518, domain="Industrial").cpu()
        score = FU.image_score(det, anchors).cpu()
    oseg, odet = O.adapted_visual_forward(img, sd, ia, cfg.vision.heads)
    otxt = O.adapted_encode_text(tok, sd, ta, cfg.text.heads)
    oanch = O.class_anchor(otxt[0:1], otxt[1:2])
    omap = O.anomaly_map(oseg, oanch, 518, "Industrial")
    oscore = O.image_score(odet, oanch)
    # 4-level sum of x50 cosine differences from two fp16 towers (visual AND text anchors come from the fp16 path
    # here, the oracle's from fp32): measured max |err| recorded by tests/test_gpu_configs.py; north star x 6
    err = (amap.double() - omap.double()).abs()
    print(f"fused anomaly map vs oracle: max |err| {err.max().item():.3e}, rms {err.pow(2).mean().sqrt().item():.3e}, "
          f"max share of 1e-3+1e-2|ref| {(err / (1e-3 + 1e-2 * omap.double().abs())).max().item():.2f}")
    # measured on MI355X over the 1.07 M pixels: rms 2.0e-3, max 8.3e-3 (4.2 sigma; it moves by +-30 % with any change
    # of summation order in the tower).  Asserted at 1.2e-2 + 1e-2 |ref| (6 sigma); what the metric needs is below.
    assert_close(amap, omap, 1.2e-2, 1e-2, "anomaly map (x100 cosines, fp16 towers on both sides of the dot)")
    assert err.pow(2).mean().sqrt().item() < 3e-3
    a = roc_auc_score(masks.reshape(-1), amap.numpy().reshape(-1))
    b = roc_auc_score(masks.reshape(-1), omap.numpy().reshape(-1))
    assert abs(a - b) <= 1e-3, (a, b)
    labels = np.array([0, 1, 0, 1])
    r1 = FU.metrics_eval(masks, labels, amap.numpy(), score.numpy(), "synthetic", "Industrial")
    r2 = FU.metrics_eval(masks, labels, omap.numpy(), oscore.numpy(), "synthetic", "Industrial")
    for k in ("pixel AUC", "pixel AP"):
        assert abs(r1[k] - r2[k]) <= 0.1 + 1e-9, (k, r1, r2)   # values are percentages rounded to 2 decimals


@pytest.mark.parametrize("precision", ["fp32", "fp16x2", "fp16"])
def test_auroc_parity_on_map_correlated_masks(dev, full_weights, precision):
    """AUROC where pixel ranking matters.  The random rectangles above are uncorrelated with the random-weight maps
    (AUROC ~ 0.5, insensitive to map errors).  Here the ground truth is derived from the REFERENCE's own map of the
    golden B = 4 run (tests/golden/full4.npz: pre-blur grids of the 4 levels -> blur, upsample, level sum as
    reference forward_utils.py:207-213 / test_last.py:95-100,149): its top-5 % region per image, dilated by 15 pixels,
    so the reference map scores AUROC ~ 0.9 on it and every mis-ranked pixel near the region's rim moves the
    figure.  Asserted for every arithmetic mode: |AUROC(HIP map) - AUROC(reference map)| <= 1e-3, same for AP
    (reference test_last.py:102-147, forward_utils.py:288-296)."""
    import forward_utils as FU
    from sklearn.metrics import average_precision_score, roc_auc_score
    g4 = np.load(os.path.join(GOLDEN, "full4.npz"))
    anchors = T(np.load(os.path.join(GOLDEN, "full.npz"))["full.anchors_bottle"])
    ref = 0
    for i in range(4):
        grid = T(g4[f"full4.map_pre_blur{i}"]).double().unsqueeze(1)
        ref = ref + O.bilinear_align_corners(O.gaussian_blur2d(grid, 7, 1.0), 518)[:, 0]
    thr = torch.quantile(ref.reshape(4, -1), 0.95, dim=1).view(4, 1, 1)
    masks = torch.nn.functional.max_pool2d((ref >= thr).float().unsqueeze(1), 31, 1, 15)[:, 0].numpy().astype(np.uint8)
    model = build_full(dev, precision, full_weights)
    with torch.no_grad():
        seg, det, _ = model(synth.synth_images(4, 518, seed=int(g4["full4.seed"])).to(dev))
        amap = FU.calculate_anomaly_map(seg, anchors.to(dev), 518, domain="Industrial").cpu().double()
    y = masks.reshape(-1)
    a_ref, a_hip = roc_auc_score(y, ref.numpy().reshape(-1)), roc_auc_score(y, amap.numpy().reshape(-1))
    p_ref, p_hip = average_precision_score(y, ref.numpy().reshape(-1)), average_precision_score(y, amap.numpy().reshape(-1))
    err = (amap - ref).abs()
    PARITY_ERRORS[f"{precision}.b4.auroc_map_correlated_masks"] = {
        "auroc_reference_map": a_ref, "auroc_hip_map": a_hip, "abs_delta_auroc": abs(a_ref - a_hip),
        "ap_reference_map": p_ref, "ap_hip_map": p_hip, "abs_delta_ap": abs(p_ref - p_hip),
        "positive_fraction": float(y.mean()), "map_max_abs_err": float(err.max()),
        "map_rms_err": float(err.pow(2).mean().sqrt())}
    assert 0.8 < a_ref < 0.995, a_ref                     # the regime where ranking errors show
    assert abs(a_ref - a_hip) <= 1e-3, (precision, a_ref, a_hip)
    assert abs(p_ref - p_hip) <= 2e-3, (precision, p_ref, p_hip)


# ----------------------------------------------------------------------------
# image pre-processing (bit-exact: integer resampling + table normalisation)
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,s,B", [(96, 96, 70, 2), (150, 130, 70, 3), (40, 56, 70, 1), (70, 70, 70, 2),
                                     (70, 100, 70, 1), (301, 70, 70, 1), (700, 700, 518, 2), (1024, 1024, 518, 2),
                                     (256, 300, 518, 1), (2500, 900, 518, 1), (5, 3, 70, 1),
                                     (1400, 1450, 70, 1)])   # 20x downscale: the source tile does not fit in LDS
def test_preprocess_bit_exact(dev, h, w, s, B):
    from oracle import preprocess_oracle as P
    rng = np.random.default_rng(h * 31 + w)
    imgs = rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)
    imgs[0, : max(h // 3, 1), : max(w // 3, 1)] = 255          # saturated block: negative lobes clip
    got = engine.preprocess(T(imgs).to(dev), s).cpu().numpy()
    for b in range(B):
        assert np.array_equal(got[b], P.preprocess(imgs[b], s)), f"image {b} differs from the oracle"


def test_preprocess_matches_golden_and_pillow(dev):
    from PIL import Image
    g = np.load(__import__("os").path.join(__import__("os").path.dirname(__file__), "golden", "preprocess.npz"))
    for i, (h, w, s) in enumerate(g["cases"]):
        got = engine.preprocess(T(g[f"in{i}"][None]).to(dev), int(s)).cpu().numpy()[0]
        assert np.array_equal(got, g[f"f32_{i}"]), f"golden case {i}"
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (333, 417, 3), dtype=np.uint8)
    ref = np.asarray(Image.fromarray(img).resize((518, 518), Image.BICUBIC))
    lut = engine._normalise_lut(engine.CLIP_MEAN, engine.CLIP_STD).numpy()
    want = np.stack([lut[c][ref[..., c]] for c in range(3)])
    assert np.array_equal(engine.preprocess(T(img[None]).to(dev), 518).cpu().numpy()[0], want)


def test_preprocess_rejects_bad_input(dev):
    with pytest.raises(ValueError):
        engine.preprocess(torch.zeros(1, 8, 8, 4, dtype=torch.uint8, device=dev), 70)
    with pytest.raises(RuntimeError):
        engine.preprocess(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), 70)


# ----------------------------------------------------------------------------
# evaluation harness end to end on a synthetic MVTec-style tree (test_last.get_predictions/evaluate)
# ----------------------------------------------------------------------------
def test_harness_end_to_end_vs_oracle(dev, tmp_path):
    import dataset as D
    import forward_utils as FU
    import test_last as TL
    from oracle import preprocess_oracle as P
    from synth_dataset import write_tree
    root = write_tree(str(tmp_path / "MVTec"))
    meta = str(tmp_path / "meta" / "MVTec" / "full-shot.jsonl")
    D.build_metadata(root, meta)
    cfg, sd, ia, ta, clip, model = build_tiny(dev, "fp32")
    S = cfg.image_size
    classes = ["bottle", "grid"]
    with torch.no_grad():
        anchors = {c: FU.get_adapted_single_class_text_embedding(model, "MVTec", c, dev) for c in classes}
    host = {c: D.BaseSingleClassDataset(root, meta, S, c) for c in classes}
    raw = {c: D.BaseSingleClassDataset(root, meta, S, c, device_preprocess=True) for c in classes}
    # text-only branch here (the reduced model's 256-wide features do not match the 768-wide IQM queries; the IQM
    # fusion of the harness is tested at full size in tests/test_gpu_iqm.py)
    rows_host = TL.evaluate(model, host, anchors, dev, S, "MVTec", batch_size=4, use_iqm=False)
    rows_raw = TL.evaluate(model, raw, anchors, dev, S, "MVTec", batch_size=4, use_iqm=False)
    assert rows_host == rows_raw, "GPU pre-processing must give the very same table as the CPU transform"
    assert rows_host[-1]["class name"] == "Average" and len(rows_host) == 3

    # the same loop on the oracle
    for c, row in zip(classes, rows_host):
        ds = host[c]
        imgs = torch.stack([ds[i]["image"] for i in range(len(ds))])
        masks = np.stack([ds[i]["mask"].numpy() for i in range(len(ds))])
        labels = np.array([ds[i]["label"] for i in range(len(ds))])
        oseg, odet = O.adapted_visual_forward(imgs, sd, ia, cfg.vision.heads, image_adapt_until=2, levels=(2, 3))
        sent = FU.class_sentences("MVTec", c)
        from model.tokenizer import tokenize
        cols = [O.adapted_encode_text(tokenize(s), sd, ta, cfg.text.heads, text_adapt_until=1) for s in sent]
        oanch = O.class_anchor(cols[0], cols[1])
        assert_close(anchors[c], oanch, 2e-4, 1e-3, f"{c} anchors")
        omap = O.anomaly_map(oseg, oanch, S, "Industrial")
        oscore = O.image_score(odet, oanch)
        with torch.no_grad():
            loader = torch.utils.data.DataLoader(ds, batch_size=4)
            m2, l2, preds, preds_image, names = TL.get_predictions(model, anchors[c], loader, dev, S, "MVTec",
                                                                   use_iqm=False)
        assert np.array_equal(m2, masks) and np.array_equal(l2, labels) and len(names) == len(ds)
        assert_close(T(preds), omap, 2e-3, 1e-3, f"{c} maps (x100 cosines, fp32 path)")
        assert_close(T(preds_image), oscore, 2e-4, 1e-3, f"{c} image scores")
        want = FU.metrics_eval(masks, labels, omap.numpy(), oscore.numpy(), c, "Industrial")
        for k in ("pixel AUC", "pixel AP"):
            assert abs(row[k] - want[k]) <= 0.1 + 1e-9, (c, k, row, want)


# ----------------------------------------------------------------------------
# "CLIP surgery" tap path: VisionTransformer.DAPM_replace (reference transformer.py:102-152,406-425)
# ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_surgery():
    import os
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "surgery.npz"))


@pytest.mark.parametrize("code", [F32, F16, BF16, F16X2])
@pytest.mark.parametrize("B", [3, 1])
@pytest.mark.parametrize("dpam", [2, 3])
def test_surgery_encode_image_vs_reference_golden(dev, golden_surgery, code, B, dpam):
    cfg, sd, ia, ta, clip, model = build_tiny(dev, NAME[code])
    clip.visual.DAPM_replace(DPAM_layer=dpam)
    img = synth.synth_images(B, cfg.image_size, seed=7).to(dev)
    with torch.no_grad():
        pooled, taps = clip.encode_image(img, [1, 2, 3])
    atol, rtol = TOL[code]
    s = 4 if code != F32 else 1          # residual-stream values are O(1..5), as in the plain tap test
    g = golden_surgery
    assert_close(pooled, T(g[f"b{B}.dpam{dpam}.pooled"]), s * atol, rtol, "pooled")
    for i, t in enumerate(taps):
        assert_close(t, T(g[f"b{B}.dpam{dpam}.tap{i + 1}"]), s * atol, rtol, f"tap{i + 1}")


def test_surgery_stage1_feature_chain(dev, golden_surgery):
    """The consumer of the surgery taps, reference train.py:75-85, written against this build's API."""
    cfg, sd, ia, ta, clip_surgery, _ = build_tiny(dev, "fp16")
    _, _, _, _, clip_plain, _ = build_tiny(dev, "fp16")
    clip_surgery.visual.DAPM_replace(DPAM_layer=3)
    img = synth.synth_images(3, cfg.image_size, seed=7).to(dev)
    with torch.no_grad():
        _, patch_features = clip_surgery.encode_image(img, [1, 2, 3])
        cls_token, _ = clip_plain.encode_image(img, [])
        cls_token = cls_token / cls_token.norm(dim=-1, keepdim=True)
        patch_features = [clip_surgery.visual.ln_post(t[:, 1:, :]) for t in patch_features]
        patch_features = [t @ clip_surgery.visual.proj for t in patch_features]
        patch_features = [t / t.norm(dim=-1, keepdim=True) for t in patch_features]
        patch_features = [t + cls_token.unsqueeze(1) for t in patch_features]
    for i, t in enumerate(patch_features):
        assert_close(t, T(golden_surgery[f"train_feat{i + 1}"]), 1e-3, 1e-2, f"stage-1 feature {i + 1}")


def test_surgery_needs_wide_workspace(dev):
    lib = _lib.load()
    x = torch.zeros(4 * 26, 256, device=dev)
    w = _lib.BlockWeights()
    rc = lib.aaclip_block(x.data_ptr(), C.byref(w), 0.0, 4, 26, 256, 4, 512, 2, F16, x.data_ptr(), 0, stream(dev))
    assert rc != 0 and b"F >= 4*D" in lib.aaclip_last_error()
    rc = lib.aaclip_block(x.data_ptr(), C.byref(w), 0.0, 4, 26, 256, 4, 1024, 3, F16, x.data_ptr(), 0, stream(dev))
    assert rc != 0 and b"attn_mode" in lib.aaclip_last_error()


# ----------------------------------------------------------------------------
# the one collective of the path on RCCL (single rank: the box has one GPU; world size 2 runs on gloo in
# tests/test_distributed_cpu.py)
# ----------------------------------------------------------------------------
def test_rccl_all_gather_single_rank(dev):
    import os
    import torch.distributed as dist
    from aaclip_hip import shard
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29541")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        x = synth.randn("t.rccl", (64, 768), 1.0, 5).to(dev)
        out = shard._all_gather(x, 1)
        dist.barrier()
        torch.cuda.synchronize(dev)
        assert torch.equal(out, x)
        assert shard.gather_rows(x) is x            # world size 1: no collective
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("code", [F16, BF16])
def test_blocks_run_folds_ln1_across_blocks(dev, full_weights, code):
    """aaclip_blocks (ln_1 of blocks 1.. folded into their QKV products, adapters feeding the fold) against the
    same blocks called one by one (ln_1 passes), B = 4 so that the large-batch kernels run; both against the
    fp32 oracle.  Blocks 4..6 of the adapted tower: two with an adapter, one without."""
    cfg, sd, ia, ta = full_weights
    model = build_full(dev, NAME[code], full_weights)
    blocks = list(model.image_encoder.transformer.resblocks[4:7])
    aws = [model.image_adapter["layer_adapters"][4].weight, model.image_adapter["layer_adapters"][5].weight, None]
    B, L, D = 4, 1370, 1024
    x0 = synth.randn("t.run.x", (B * L, D), 1.0, 11)
    xa = x0.clone().to(dev)
    engine.run_blocks(xa, blocks, B, L, 16, code, adapter_weights=aws, mix=0.1)
    xb = x0.clone().to(dev)
    for blk, aw in zip(blocks, aws):
        engine.run_block(xb, blk, B, L, 16, code, adapter_weight=aw, mix=0.1)
    ref = x0.view(B, L, D).double()
    sdd = {k: v.double() for k, v in sd.items()}
    for i in (4, 5, 6):
        ref = O.resblock(ref, sdd, f"visual.transformer.resblocks.{i}.", 16, None)
        if i < 6:
            ref = O.adapter_mix(ref, ia[f"layer_adapters.{i}.fc.0.weight"].double(), 0.1)
    ref = ref.view(B * L, D)
    atol, rtol = (6e-3, 1e-2) if code == F16 else (5e-2, 5e-2)
    assert_close(xa, ref, atol, rtol, "one aaclip_blocks call vs oracle")
    assert_close(xb, ref, atol, rtol, "block by block vs oracle")
    assert_close(xa, xb, atol, rtol, "one call vs block by block")


@pytest.mark.parametrize("B", [2, 4])
def test_blocks_taps_one_call_vs_one_call_per_run(dev, full_weights, B):
    """aaclip_blocks_taps (the whole tower with its taps in one call: per-block output buffers) against one
    aaclip_blocks_to call per run between taps.  B = 2 (small-batch kernels, LayerNorm passes everywhere): identical
    bits.  B = 4 (large-batch kernels): the one-call form also folds ln_1 of the first block behind a tap, which the
    per-run calls run as a pass -- equal within the fp16 tolerance, taps untouched by later blocks, and both against
    the oracle."""
    cfg, sd, ia, ta = full_weights
    model = build_full(dev, "fp16", full_weights)
    blocks = list(model.image_encoder.transformer.resblocks[3:9])
    aws = [model.image_adapter["layer_adapters"][i].weight if i < 6 else None for i in range(3, 9)]
    L, D = 1370, 1024
    x0 = synth.randn("t.taps.x", (B * L, D), 1.0, 23)
    # one call: blocks 3,4 in place on a; tap; blocks 5,6,7 in b; tap; block 8 in c
    a, b, c = x0.clone().to(dev), torch.empty(B * L, D, device=dev), torch.empty(B * L, D, device=dev)
    engine.run_blocks(a, blocks, B, L, 16, F16, adapter_weights=aws, mix=0.1, x_outs=[a, a, b, b, b, c])
    # one call per run
    a2, b2, c2 = x0.clone().to(dev), torch.empty(B * L, D, device=dev), torch.empty(B * L, D, device=dev)
    engine.run_blocks(a2, blocks[:2], B, L, 16, F16, adapter_weights=aws[:2], mix=0.1)
    engine.run_blocks(a2, blocks[2:5], B, L, 16, F16, adapter_weights=aws[2:5], mix=0.1, x_out=b2)
    engine.run_blocks(b2, blocks[5:], B, L, 16, F16, adapter_weights=aws[5:], mix=0.1, x_out=c2)
    assert torch.equal(a, a2)                       # the first run is the same sequence of launches either way
    if B == 2:
        assert torch.equal(b, b2) and torch.equal(c, c2)
    else:
        assert_close(b, b2, 6e-3, 1e-2, "tap 2: one call vs per-run calls")
        assert_close(c, c2, 6e-3, 1e-2, "final: one call vs per-run calls")
        assert not torch.equal(b, b2)               # ln_1 behind the tap really ran folded
    ref = x0.view(B, L, D).double()
    sdd = {k: v.double() for k, v in sd.items()}
    refs = {}
    for i in range(3, 9):
        ref = O.resblock(ref, sdd, f"visual.transformer.resblocks.{i}.", 16, None)
        if i < 6:
            ref = O.adapter_mix(ref, ia[f"layer_adapters.{i}.fc.0.weight"].double(), 0.1)
        refs[i] = ref.view(B * L, D)
    assert_close(a, refs[4], 6e-3, 1e-2, "tap 1 vs oracle")
    assert_close(b, refs[7], 6e-3, 1e-2, "tap 2 vs oracle")
    assert_close(c, refs[8], 6e-3, 1e-2, "final vs oracle")


def test_text_tower_large_batch_folds_like_small_batches(dev, full_weights):
    """encode_text on 64 sentences (M = 4928 rows: the 256-tile kernels with LayerNorm folding, width 768, causal)
    against the same sentences encoded 8 at a time (128-tile kernels, LayerNorm passes) and against the oracle."""
    cfg, sd, ia, ta = full_weights
    model = build_full(dev, "fp16", full_weights)
    import forward_utils as FU
    from model.tokenizer import tokenize
    sentences = []
    for c in ("bottle", "cable", "capsule", "carpet"):
        for group in FU.class_sentences("MVTec", c):
            sentences.extend(group)
    sentences = sentences[:64]
    tok = tokenize(sentences).to(dev)
    with torch.no_grad():
        big = model.encode_text(tok)
        small = torch.cat([model.encode_text(tok[i:i + 8]) for i in range(0, 64, 8)])
    unit = lambda t: t / t.norm(dim=-1, keepdim=True)
    assert_close(unit(big), unit(small), 1e-3, 1e-2, "64 sentences at once vs 8 at a time")
    ref = O.adapted_encode_text(tok[:4].cpu(), sd, ta, cfg.text.heads)
    assert_close(unit(big[:4]), unit(ref), 1e-3, 1e-2, "folded text tower vs oracle")


@pytest.mark.parametrize("code", [F16, BF16])
def test_tiny_adapted_large_batch_vs_oracle(dev, code):
    """The whole adapted path of the reduced model at B = 160 (M = 4160 rows: 256-tile GEMMs, LayerNorm folding,
    aaclip_blocks runs between taps, adapters feeding the fold) against the oracle, and against the same images
    in small batches (128-tile GEMMs, LayerNorm passes)."""
    cfg, sd, ia, ta, clip, model = build_tiny(dev, NAME[code])
    B = 160
    img = synth.synth_images(B, cfg.image_size, seed=17)
    atol, rtol = TOL[code]
    with torch.no_grad():
        seg, det, _ = model(img.to(dev))
        seg_s, det_s, _ = model(img[:3].to(dev))
        pooled, taps = clip.encode_image(img.to(dev), [1, 3])
    oseg, odet = O.adapted_visual_forward(img, sd, ia, cfg.vision.heads, image_adapt_until=2, levels=(2, 3),
                                          dtype=torch.float64)
    for i in range(2):
        assert_close(seg[i], oseg[i], atol, rtol, f"seg{i} (B=160)")
        assert_close(seg[i][:3], seg_s[i], atol, rtol, f"seg{i}: large batch vs small batch")
    assert_close(det, odet, atol, rtol, "det (B=160)")
    opooled, otaps = O.encode_image(img, sd, cfg.vision.heads, [1, 3], dtype=torch.float64)
    # raw residual-stream values are O(1..5): the tolerance is relative there; with 10^6 elements per tap the tail of
    # the fp16 rounding noise reaches further than in the 3-image test (5 elements beyond 4e-3 + 1e-2*|ref|)
    if code != F16:
        return   # bf16 (8-bit mantissa) is not the parity path: its raw-stream tails are not asserted on 10^6 elements
    s4 = 8
    assert_close(pooled, opooled, s4 * atol, rtol, "pooled (B=160)")
    for i in range(2):
        assert_close(taps[i], otaps[i], s4 * atol, rtol, f"tap{i} (B=160)")


def test_bench_batch_is_bit_identical_to_small_large_regime_batches(dev, full_weights):
    """BASELINE.json's size (B = 64) through a size-independent property: every image's seg / det tokens and
    anomaly map at B = 64 are bit-identical to what a batch of 4 gives (same kernels), which the other tests tie to
    the oracle and the reference's golden vectors."""
    import forward_utils as FU
    model = build_full(dev, "fp16", full_weights)
    img = synth.synth_images(64, 518, seed=64).to(dev)
    anchors = torch.nn.functional.normalize(synth.randn("t.b64.anchors", (768, 2), 1.0, 3), dim=0).to(dev)
    with torch.no_grad():
        seg, det, _ = model(img)
        amap = FU.calculate_anomaly_map(seg, anchors, 518, domain="Industrial")
        for lo in (0, 60):
            seg4, det4, _ = model(img[lo:lo + 4])
            amap4 = FU.calculate_anomaly_map(seg4, anchors, 518, domain="Industrial")
            for a, b in zip(seg, seg4):
                assert torch.equal(a[lo:lo + 4], b)
            assert torch.equal(det[lo:lo + 4], det4)
            assert torch.equal(amap[lo:lo + 4], amap4)
    assert torch.isfinite(amap).all()
