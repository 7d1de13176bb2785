"""Shapes, inputs and fp64 references shared by tests/test_visual_backward_cpu.py and tests/test_gpu_visual_backward.py
(the tiled attention backward, the block backward at visual shapes, autograd.visual_taps)."""
import functools

import torch

import oracle.aaclip_oracle as O
from aaclip_hip import synth

# (B, H, L): below one 32-row tile, exactly one, one row into the second 128-query workgroup, a multiple of 128, one
# past it, and the visual length (42 full key tiles + 26 rows).  L <= 128 reaches the tiled kernels with long_rows=True.
ATTENTION_CASES = [(1, 1, 1), (2, 4, 31), (1, 2, 32), (3, 4, 77), (2, 4, 128), (1, 1, 129), (2, 4, 160), (1, 4, 256),
                   (2, 16, 257), (1, 2, 1370)]
VISUAL_L, VISUAL_H = 1370, 16

# The inputs are drawn from the case's name.  With an adapter the reference's derivative is discontinuous where an adapter
# pre-activation z is 0 (LeakyReLU), so a case must keep every |z| above the fp32 error of z (~1e-6 at z rms 1.3): one
# element inside it (z = -2.9e-7, drawn by an earlier name of the d_in = None case) is computed on the other side of
# the kink in fp32 and alone moves d_adapter_w by 9.1e-5.  Smallest |z| of the cases below, in fp64: 3.3e-6 (at width
# 256), 4.1e-6 and 9.9e-6.
# name -> (width: "tiny" = 256 / 4 heads / 1024, "full" = 1024 / 16 heads / 4096; B, L, causal, adapter, alias, d_in)
BLOCK_CASES = {
    "visual_length_reduced_width": ("tiny", 1, 1370, False, True, False, True),
    "full_width_adapter_alias": ("full", 2, 170, False, True, True, True),
    "full_width_adapter_weight_only": ("full", 2, 170, False, True, False, False),
    "full_width_plain": ("full", 2, 170, False, False, False, True),
    "causal": ("tiny", 2, 160, True, True, False, True),
}

TAPS_IMAGE, TAPS_UNTIL, TAPS_LEVELS, TAPS_BATCH, TAPS_MIX = 182, 2, [2, 3], 2, 0.1     # grid 13: L = 170 > 128


def rnd(name, shape, std=1.0):
    return synth.randn("vb." + name, shape, std, 29)


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.isfinite(a).all()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def attention_inputs(B, H, L, peak=None):
    """-> (qkv [B*L, 3*64*H] with q pre-scaled, d_ctx [B*L, 64*H]) in fp32.  peak: rescale every q row so that its
    largest score is `peak`."""
    D = 64 * H
    qkv = rnd(f"attn.qkv.{B}.{L}.{H}", (B * L, 3 * D))
    qkv[:, :D] *= 0.5
    d_ctx = rnd(f"attn.dctx.{B}.{L}.{H}", (B * L, D))
    if peak is not None:
        q, k, _ = (t.reshape(B, L, H, 64).transpose(1, 2) for t in qkv.double().split(D, dim=-1))
        top = (q @ k.transpose(-1, -2)).amax(dim=-1)               # [B, H, L]
        assert (top > 0).all()
        scale = (peak / top).transpose(1, 2).reshape(B * L, H, 1)
        qkv[:, :D] = (qkv[:, :D].double().reshape(B * L, H, 64) * scale).reshape(B * L, D).float()
    return qkv, d_ctx


def attention_reference(qkv, d_ctx, B, H, L, causal):
    """fp64 autograd of softmax(q k^T) v -> d qkv [B*L, 3*64*H]"""
    D = 64 * H
    x = qkv.double().requires_grad_(True)
    q, k, v = (t.reshape(B, L, H, 64).transpose(1, 2) for t in x.split(D, dim=-1))
    s = q @ k.transpose(-1, -2)
    if causal:
        s = s + O.causal_mask(L, torch.float64)
    ctx = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B * L, D)
    ctx.backward(d_ctx.double())
    return x.grad


@functools.lru_cache(maxsize=None)
def attention_case(B, H, L, causal):
    """-> (qkv, d_ctx, fp64 d qkv): computed once, shared, never modified"""
    qkv, d_ctx = attention_inputs(B, H, L)
    return qkv, d_ctx, attention_reference(qkv, d_ctx, B, H, L, causal)


def taps_cfg():
    cfg = synth.tiny_cfg()
    cfg.image_size = TAPS_IMAGE
    return cfg


def full_width_cfg():
    return synth.ClipCfg(embed_dim=256, image_size=70, vision=synth.TowerCfg(1024, 1, 16, 4096),
                         text=synth.TowerCfg(256, 1, 4, 1024))


def build_clip(cfg, precision, seed):
    from model.model import CLIP
    sd = synth.synth_clip_state_dict(cfg, seed=seed)
    clip = CLIP(cfg.embed_dim,
                dict(image_size=cfg.image_size, layers=cfg.vision.layers, width=cfg.vision.width,
                     patch_size=cfg.patch_size),
                dict(context_length=77, vocab_size=cfg.vocab_size, width=cfg.text.width, heads=cfg.text.heads,
                     layers=cfg.text.layers), precision=precision)
    clip.load_state_dict(sd, strict=True)
    return sd, clip


def build_taps_model(dev, precision):
    """The reduced model at image size 182 with seeded image-adapter weights; only the layer adapters train."""
    from model.adapter import AdaptedCLIP
    cfg = taps_cfg()
    sd, clip = build_clip(cfg, precision, 7)
    ia = synth.synth_image_adapter_state_dict(cfg, until=TAPS_UNTIL, levels=len(TAPS_LEVELS), relu=False, seed=7)
    model = AdaptedCLIP(clip, text_adapt_until=1, image_adapt_until=TAPS_UNTIL, levels=TAPS_LEVELS, relu=False,
                        image_adapt_weight=TAPS_MIX)
    model.image_adapter.load_state_dict(ia, strict=True)
    for p in model.parameters():
        p.requires_grad_(False)
    for p in model.image_adapter["layer_adapters"].parameters():
        p.requires_grad_(True)
    return cfg, sd, ia, model.to(dev).eval()


def taps_inputs():
    """-> (images [B, 3, S, S] fp32, mask [B, 1, S, S] fp64, anchors [E, 2] fp64 with unit columns)"""
    S = TAPS_IMAGE
    image = synth.synth_images(TAPS_BATCH, S, seed=7)
    mask = torch.zeros(TAPS_BATCH, 1, S, S, dtype=torch.float64)
    for b in range(TAPS_BATCH):
        y, x = 15 + 31 * b, 22 + 19 * b
        mask[b, 0, y:y + S // 3, x:x + S // 2] = 1
    t = rnd("taps.anchors", (256, 2)).double()
    return image, mask, t / t.norm(dim=0, keepdim=True)
