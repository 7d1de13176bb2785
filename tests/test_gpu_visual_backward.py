"""Backward through the visual blocks on the GPU: the tiled attention backward (csrc/attention_backward.hip), the block
backward at visual shapes (aaclip_block_backward_long) and aaclip_hip.autograd.visual_taps.

Bars, the project's own (tests/test_gpu_text_backward.py).  Building blocks and the block backward against fp64 torch
autograd: 1e-4 relative Frobenius.  Whole-model gradients with precision fp32: at most 8 x e_ref, e_ref being the
oracle's own fp32 CPU autograd against its fp64 autograd, computed in the same test.  precision fp16x2: 1e-2.
Every measured error goes to PARITY_ERRORS under visual_backward.*"""
import pytest
import torch

import forward_utils as FU
import oracle.aaclip_oracle as O
import visual_backward_cases as VB
from aaclip_hip import _lib, autograd, engine, synth
from conftest import PARITY_ERRORS
from seg_loss_cases import seg_loss_terms, similarity_map
from visual_backward_cases import rel, rnd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------- attention backward
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("B,H,L", VB.ATTENTION_CASES)
def test_attention_backward_long(dev, B, H, L, causal):
    qkv, d_ctx, want = VB.attention_case(B, H, L, causal)
    got = engine.attention_backward(qkv.to(dev), d_ctx.to(dev), B, L, H, causal, long_rows=True)
    D = 64 * H
    errs = {"dq": rel(got[:, :D], want[:, :D]), "dk": rel(got[:, D:2 * D], want[:, D:2 * D]),
            "dv": rel(got[:, 2 * D:], want[:, 2 * D:]), "all": rel(got, want)}
    print("attention_long", B, H, L, causal, errs)
    PARITY_ERRORS[f"visual_backward.attention.{'causal' if causal else 'full'}.B{B}.H{H}.L{L}"] = errs
    assert all(v <= 1e-4 for v in errs.values()), errs
    if L > 128:        # long_rows=None chooses the tiled kernels by itself above 128 tokens
        assert torch.equal(engine.attention_backward(qkv.to(dev), d_ctx.to(dev), B, L, H, causal), got)


def test_attention_backward_long_peaked_rows(dev):
    """Largest score of every row ~ 30 (DESIGN 10's range); image 1 has an all-zero d_ctx."""
    B, H, L = 2, 4, 257
    D = 64 * H
    qkv, d_ctx = VB.attention_inputs(B, H, L, peak=30.0)
    d_ctx[L:] = 0
    want = VB.attention_reference(qkv, d_ctx, B, H, L, False)
    got = engine.attention_backward(qkv.to(dev), d_ctx.to(dev), B, L, H, False)
    errs = {"dq": rel(got[:L, :D], want[:L, :D]), "dk": rel(got[:L, D:2 * D], want[:L, D:2 * D]),
            "dv": rel(got[:L, 2 * D:], want[:L, 2 * D:])}
    print("attention_long peaked", errs)
    PARITY_ERRORS["visual_backward.attention.peaked.B2.H4.L257"] = errs
    assert torch.isfinite(got).all()
    assert not got[L:].any()                     # exactly zero: dq, dk and dv of the image without a gradient
    assert all(v <= 1e-4 for v in errs.values()), errs


def test_attention_backward_long_dq_scale(dev):
    B, H, L = 2, 4, 257
    D = 64 * H
    qkv, d_ctx, want = VB.attention_case(B, H, L, False)
    got = engine.attention_backward(qkv.to(dev), d_ctx.to(dev), B, L, H, False)
    got2 = engine.attention_backward(qkv.to(dev), d_ctx.to(dev), B, L, H, False, dq_scale=0.125)
    assert torch.equal(got2[:, D:], got[:, D:])
    e = rel(got2[:, :D], 0.125 * want[:, :D])
    PARITY_ERRORS["visual_backward.attention.dq_scale.B2.H4.L257"] = e
    assert e <= 1e-4, e


def test_attention_backward_long_is_deterministic(dev):
    B, H, L = 1, 2, 1370
    qkv, d_ctx, _ = VB.attention_case(B, H, L, False)
    a = engine.attention_backward(qkv.to(dev), d_ctx.to(dev), B, L, H, False)
    b = engine.attention_backward(qkv.to(dev), d_ctx.to(dev), B, L, H, False)
    assert torch.equal(a, b)


def test_short_rows_keep_the_old_path(dev):
    B, H, L = 3, 4, 77
    qkv, d_ctx, _ = VB.attention_case(B, H, L, True)
    q, d = qkv.to(dev), d_ctx.to(dev)
    direct = torch.empty_like(q)
    _lib.check(_lib.load().aaclip_attention_backward(q.data_ptr(), d.data_ptr(), direct.data_ptr(), B, L, H, 1, 1.0,
                                                     None), "attention_backward")
    torch.cuda.synchronize()
    assert torch.equal(engine.attention_backward(q, d, B, L, H, True), direct)
    assert torch.equal(engine.attention_backward(q, d, B, L, H, True, long_rows=None), direct)


# ---------------------------------------------------------------------------------------------- block backward
@pytest.fixture(scope="module")
def block_models(dev):
    out = {}
    for width, cfg in (("tiny", synth.tiny_cfg()), ("full", VB.full_width_cfg())):
        sd, clip = VB.build_clip(cfg, "fp32", 7)
        out[width] = (cfg, sd, clip.to(dev).eval())
    return out


@pytest.mark.parametrize("case", list(VB.BLOCK_CASES))
def test_block_backward_long(dev, block_models, case):
    width, B, L, causal, adapter, alias, want_d_in = VB.BLOCK_CASES[case]
    cfg, sd, clip = block_models[width]
    D, H, mix = cfg.vision.width, cfg.vision.heads, 0.1
    block = clip.visual.transformer.resblocks[0]
    pre = "visual.transformer.resblocks.0."
    x = rnd(f"blk.x.{case}", (B * L, D))
    d_out = rnd(f"blk.do.{case}", (B * L, D))
    aw = synth._xavier(f"vb.blk.adapter.{D}", D, D, 29) if adapter else None
    sd64 = {k: v.double() for k, v in sd.items() if k.startswith(pre)}
    x64 = x.double().reshape(B, L, D).requires_grad_(True)
    y = O.resblock(x64, sd64, pre, H, O.causal_mask(L, torch.float64) if causal else None)
    a64 = None
    if adapter:
        a64 = aw.double().requires_grad_(True)
        y = O.adapter_mix(y, a64, mix)
    y.backward(d_out.double().reshape(B, L, D))
    d_dev = d_out.to(dev)
    aw_dev = torch.nn.Parameter(aw.to(dev), requires_grad=False) if adapter else None
    d_in, d_aw = engine.block_backward(x.to(dev), block, B, L, H, d_dev, causal=causal, adapter_weight=aw_dev, mix=mix,
                                       need_input_grad=want_d_in, in_place=alias)
    errs = {}
    if not want_d_in:
        assert d_in is None
    else:
        if alias:
            assert d_in.data_ptr() == d_dev.data_ptr()
        errs["d_in"] = rel(d_in, x64.grad.reshape(B * L, D))
    if adapter:
        errs["d_adapter_w"] = rel(d_aw, a64.grad)
    else:
        assert d_aw is None
    print("block_long", case, errs)
    PARITY_ERRORS[f"visual_backward.block.{case}"] = errs
    assert all(v <= 1e-4 for v in errs.values()), errs


# ---------------------------------------------------------------------------------------------- visual_taps
def adapter_params(model):
    return [m.weight for m in model.image_adapter["layer_adapters"]]


def hip_loss(model, image, mask, anchors):
    """The heads of AdaptedCLIP.forward composed from torch ops on the tap streams (oracle.adapted_visual_forward: drop
    CLS, ln_post, seg_proj, normalise), then the stage's map + segmentation loss per level, summed."""
    v = model.image_encoder
    loss = 0
    for k, tap in enumerate(autograd.visual_taps(model, image)):
        t = torch.nn.functional.layer_norm(tap[:, 1:, :], (tap.shape[-1],), v.ln_post.weight, v.ln_post.bias, 1e-5)
        seg = torch.nn.functional.normalize(t @ model.image_adapter["seg_proj"][k].weight.t(), dim=-1)
        loss = loss + FU.calculate_seg_loss(FU.calculate_similarity_map(seg, anchors, VB.TAPS_IMAGE), mask)
    return loss


def oracle_run(cfg, sd, ia, image, mask, anchors, dtype):
    leaves = {k: v.to(dtype) for k, v in ia.items()}
    keys = [f"layer_adapters.{i}.fc.0.weight" for i in range(VB.TAPS_UNTIL)]
    for k in keys:
        leaves[k].requires_grad_(True)
    seg, _, streams = O.adapted_visual_forward(image, sd, leaves, cfg.vision.heads, VB.TAPS_MIX, VB.TAPS_UNTIL,
                                               VB.TAPS_LEVELS, relu=False, dtype=dtype, return_stream=True)
    loss = sum(sum(seg_loss_terms(similarity_map(s, anchors.to(dtype), VB.TAPS_IMAGE), mask.to(dtype))) for s in seg)
    loss.backward()
    return loss.item(), [leaves[k].grad for k in keys], [s.detach() for s in streams]


def taps_gradient_errors(dev, precision, with_ref):
    cfg, sd, ia, model = VB.build_taps_model(dev, precision)
    image, mask, anchors = VB.taps_inputs()
    loss64, g64, streams64 = oracle_run(cfg, sd, ia, image, mask, anchors, torch.float64)
    e_ref = None
    if with_ref:
        _, g32, _ = oracle_run(cfg, sd, ia, image, mask, anchors, torch.float32)
        e_ref = [rel(a, b) for a, b in zip(g32, g64)]
    with torch.no_grad():
        e_taps = [rel(t, s) for t, s in zip(autograd.visual_taps(model, image.to(dev)), streams64)]
    loss = hip_loss(model, image.to(dev), mask.float().to(dev), anchors.float().to(dev))
    loss.backward()
    e_hip = [rel(p.grad, g) for p, g in zip(adapter_params(model), g64)]
    for p in model.parameters():
        assert p.grad is None or any(p is q for q in adapter_params(model))
    return abs(loss.item() - loss64) / abs(loss64), e_taps, e_hip, e_ref


def test_visual_taps_gradients_fp32(dev):
    e_loss, e_taps, e_hip, e_ref = taps_gradient_errors(dev, "fp32", True)
    print("visual_taps fp32: loss", e_loss, "taps", e_taps, "hip", e_hip, "ref", e_ref)
    PARITY_ERRORS["visual_backward.taps.fp32"] = {"loss_rel": e_loss, "taps": e_taps, "e_hip": e_hip, "e_ref": e_ref}
    for h, r in zip(e_hip, e_ref):
        assert h <= 8 * r, (e_hip, e_ref)


def test_visual_taps_gradients_fp16x2(dev):
    e_loss, e_taps, e_hip, _ = taps_gradient_errors(dev, "fp16x2", False)
    print("visual_taps fp16x2: loss", e_loss, "taps", e_taps, "hip", e_hip)
    PARITY_ERRORS["visual_backward.taps.fp16x2"] = {"loss_rel": e_loss, "taps": e_taps, "e_hip": e_hip}
    for h in e_hip:
        assert h <= 1e-2, e_hip


def test_taps_are_those_of_the_no_grad_path(dev):
    for precision in ("fp32", "fp16x2"):
        cfg, sd, ia, model = VB.build_taps_model(dev, precision)
        image = VB.taps_inputs()[0].to(dev)
        v = model.image_encoder
        with torch.no_grad():      # what AdaptedCLIP.forward feeds its heads
            code = model._code()
            xs, B, L = engine.patch_embed(image, v, code)
            aws = [m.weight for m in model.image_adapter["layer_adapters"]] + [None]
            _, ref = v.transformer.run(xs, B, L, code, False, VB.TAPS_LEVELS, adapter_weights=aws, mix=model.i_w)
            plain = autograd.visual_taps(model, image)
        taps = autograd.visual_taps(model, image)
        assert len(taps) == len(ref) == len(VB.TAPS_LEVELS)
        for t, p, r in zip(taps, plain, ref):
            assert t.shape == (B, L, cfg.vision.width) and L == 170
            assert t.grad_fn is not None and p.grad_fn is None
            assert torch.equal(t.detach().reshape(B * L, -1), r), precision
            assert torch.equal(p.reshape(B * L, -1), r), precision


def test_two_backward_passes_are_bit_identical(dev):
    cfg, sd, ia, model = VB.build_taps_model(dev, "fp32")
    image, mask, anchors = VB.taps_inputs()
    image, mask, anchors = image.to(dev), mask.float().to(dev), anchors.float().to(dev)
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        hip_loss(model, image, mask, anchors).backward()
        runs.append([p.grad.clone() for p in adapter_params(model)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_saved_streams_are_freed(dev):
    cfg, sd, ia, model = VB.build_taps_model(dev, "fp32")
    image = VB.taps_inputs()[0].to(dev)
    sum(t.sum() for t in autograd.visual_taps(model, image)).backward()     # warm the workspace and the weight caches
    model.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    taps = autograd.visual_taps(model, image)
    unit = VB.TAPS_BATCH * 170 * cfg.vision.width * 4
    assert torch.cuda.memory_allocated(dev) >= base + 4 * unit      # the patch-embed output and the three streams
    sum(t.sum() for t in taps).backward()
    del taps
    model.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(dev) == base


def test_backward_stops_at_the_first_trainable_adapter(dev):
    cfg, sd, ia, model = VB.build_taps_model(dev, "fp32")
    image = VB.taps_inputs()[0].to(dev)
    probe = [rnd(f"taps.probe.{k}", (VB.TAPS_BATCH, 170, cfg.vision.width)).to(dev) for k in range(2)]

    def run():
        model.zero_grad(set_to_none=True)
        sum((t * w).sum() for t, w in zip(autograd.visual_taps(model, image), probe)).backward()
        return [None if p.grad is None else p.grad.clone() for p in adapter_params(model)]

    full = run()
    adapter_params(model)[0].requires_grad_(False)
    part = run()
    assert part[0] is None                          # block 0 is not revisited
    assert rel(part[1], full[1]) <= 1e-6
    adapter_params(model)[1].requires_grad_(False)  # nothing trainable: no graph, nothing saved
    assert all(t.grad_fn is None for t in autograd.visual_taps(model, image))


def test_cpu_tensors_still_raise(dev):
    cfg, sd, ia, model = VB.build_taps_model(torch.device("cpu"), "fp32")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        autograd.visual_taps(model, VB.taps_inputs()[0])
