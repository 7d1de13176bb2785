"""The bf16x3 backward of the visual blocks on the GPU (csrc/split3_rows.hip, csrc/attention_backward_bf16x3.hip,
aaclip_block_backward_long_bf16x3, autograd.use_backward_precision).

Bars.  split3 rows: bit for bit torch's bfloat16 planes.  Attention and block backward against fp64 torch autograd: 1e-4
relative Frobenius, the bar of tests/test_gpu_visual_backward.py for the fp32 entries (the arithmetic's own emulation
stays below 3.6e-5 on these inputs: tests/test_backward_bf16x3_cpu.py).  Whole model: forward outputs and loss bit-equal
to the run under the fp32 backward; adapter gradients against the fp64 oracle 1e-2, the project's bar for its non-exact
mode (test_visual_taps_gradients_fp16x2) -- 87 040 adapter pre-activations cannot all be kept off the LeakyReLU kink,
and one flipped element is worth about 1e-3 there.  Every measured error goes to PARITY_ERRORS under backward_bf16x3.*"""
import ctypes as C

import pytest
import torch

import backward_bf16x3_cases as BC
import forward_utils as FU
import head_backward_cases as HB
import oracle.aaclip_oracle as O
import visual_backward_cases as VB
from aaclip_hip import _lib, autograd, engine, synth
from backward_bf16x3_cases import BAR, rel, rnd
from conftest import PARITY_ERRORS
from seg_loss_cases import seg_loss_terms, similarity_map

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------- split3 rows
@pytest.mark.parametrize("rows,K", BC.SPLIT_SHAPES)
def test_split3_rows_bit_for_bit(dev, rows, K):
    for name, x in BC.split_inputs(rows, K):
        got = engine.split3_rows(x.to(dev))
        assert got.dtype == torch.bfloat16 and got.shape == (rows, 3 * K)
        want = BC.split_planes(x)
        assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16)), (name, rows, K)
        assert not got[rows // 2].any()


# ---------------------------------------------------------------------------------------------- attention backward
def run_attention(dev, qkv, d_ctx, B, H, L, causal, **kw):
    return engine.attention_backward(qkv.to(dev), d_ctx.to(dev), B, L, H, causal, precision="bf16x3", **kw)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("B,H,L", BC.ATTENTION_CASES)
def test_attention_backward(dev, B, H, L, causal):
    qkv, d_ctx, want = VB.attention_case(B, H, L, causal)
    errs = BC.attention_errors(run_attention(dev, qkv, d_ctx, B, H, L, causal), want, H)
    print("attention bf16x3", B, H, L, causal, errs)
    PARITY_ERRORS[f"backward_bf16x3.attention.{'causal' if causal else 'full'}.B{B}.H{H}.L{L}"] = errs
    assert all(v <= BAR for v in errs.values()), errs


def test_attention_backward_peaked_rows(dev):
    B, H, L, _ = BC.PEAKED
    qkv, d_ctx, want = BC.peaked_case()
    got = run_attention(dev, qkv, d_ctx, B, H, L, False)
    errs = BC.attention_errors(got, want, H, rows=L)
    print("attention bf16x3 peaked", errs)
    PARITY_ERRORS["backward_bf16x3.attention.peaked.B2.H4.L257"] = errs
    assert torch.isfinite(got).all()
    assert not got[L:].any()                     # exactly zero: dq, dk and dv of the image without a gradient
    assert all(v <= BAR for v in errs.values()), errs


def test_attention_backward_dq_scale(dev):
    B, H, L = 2, 4, 160
    D = 64 * H
    qkv, d_ctx, want = VB.attention_case(B, H, L, False)
    got = run_attention(dev, qkv, d_ctx, B, H, L, False)
    got2 = run_attention(dev, qkv, d_ctx, B, H, L, False, dq_scale=0.125)
    assert torch.equal(got2[:, D:], got[:, D:])
    e = rel(got2[:, :D], 0.125 * want[:, :D])
    PARITY_ERRORS["backward_bf16x3.attention.dq_scale.B2.H4.L160"] = e
    assert e <= BAR, e


def test_attention_backward_is_deterministic(dev):
    B, H, L = 1, 2, 1370
    qkv, d_ctx, _ = VB.attention_case(B, H, L, False)
    assert torch.equal(run_attention(dev, qkv, d_ctx, B, H, L, False), run_attention(dev, qkv, d_ctx, B, H, L, False))


def test_attention_backward_keeps_the_range(dev):
    """d_ctx * 2^-40: fp16 operands see zeros (tests/test_backward_bf16x3_cpu.py); bf16 has fp32's exponent"""
    B, H, L, _ = BC.RANGE
    qkv, small, want = BC.range_case()
    errs = BC.attention_errors(run_attention(dev, qkv, small, B, H, L, False), want, H)
    print("attention bf16x3 range", errs)
    PARITY_ERRORS["backward_bf16x3.attention.range.B2.H4.L160"] = errs
    assert all(v <= BAR for v in errs.values()), errs


def test_attention_backward_is_a_path_of_its_own(dev):
    B, H, L = 2, 4, 160
    qkv, d_ctx, _ = VB.attention_case(B, H, L, False)
    q, d = qkv.to(dev), d_ctx.to(dev)
    plain = engine.attention_backward(q, d, B, L, H, False)
    assert torch.equal(engine.attention_backward(q, d, B, L, H, False, precision="fp32"), plain)
    direct = torch.empty_like(q)
    lib = _lib.load()
    ws = torch.empty(lib.aaclip_attention_backward_long_workspace_bytes(B, L, H), dtype=torch.uint8, device=dev)
    _lib.check(lib.aaclip_attention_backward_long(q.data_ptr(), d.data_ptr(), direct.data_ptr(), B, L, H, 0, 1.0,
                                                  ws.data_ptr(), ws.numel(), None), "attention_backward_long")
    torch.cuda.synchronize()
    assert torch.equal(plain, direct)                               # the fp32 entry, as before
    assert not torch.equal(run_attention(dev, qkv, d_ctx, B, H, L, False), plain)
    B, H, L = 3, 4, 77                                              # bf16x3 takes the tiled entry at any L
    qkv, d_ctx, want = VB.attention_case(B, H, L, True)
    short = engine.attention_backward(qkv.to(dev), d_ctx.to(dev), B, L, H, True)
    assert not torch.equal(run_attention(dev, qkv, d_ctx, B, H, L, True), short)


# ---------------------------------------------------------------------------------------------- block backward
@pytest.fixture(scope="module")
def block_models(dev):
    out = {}
    for width in ("tiny", "full"):
        cfg = BC.block_cfg(width)
        sd, clip = BC.build_clip(cfg, "fp32", 7)
        out[width] = (cfg, sd, clip.to(dev).eval())
    return out


@pytest.mark.parametrize("case", list(BC.PLAIN_BLOCK_CASES))
def test_block_backward_without_adapter(dev, block_models, case):
    width, B, L, causal = BC.PLAIN_BLOCK_CASES[case]
    cfg, sd, clip = block_models[width]
    D, H = cfg.vision.width, cfg.vision.heads
    x, d_out = rnd(f"blk.x.{case}", (B * L, D)), rnd(f"blk.do.{case}", (B * L, D))
    want, _, _ = BC.block_reference(sd, cfg, x, d_out, B, L, causal)
    d_in, d_aw = engine.block_backward(x.to(dev), clip.visual.transformer.resblocks[0], B, L, H, d_out.to(dev),
                                       causal=causal, precision="bf16x3")
    assert d_aw is None
    errs = {"d_in": rel(d_in, want)}
    print("block bf16x3", case, errs)
    PARITY_ERRORS[f"backward_bf16x3.block.{case}"] = errs
    assert errs["d_in"] <= BAR, errs


@pytest.mark.parametrize("want_d_in,alias", [(True, False), (False, False), (True, True)])
def test_block_backward_with_adapter(dev, block_models, want_d_in, alias):
    c = BC.ADAPTER_CASE
    cfg, sd, x, d_out, aw, want_dx, want_daw, _ = BC.adapter_case()
    clip = block_models[c["width"]][2]
    d_dev = d_out.to(dev)
    aw_dev = torch.nn.Parameter(aw.to(dev), requires_grad=False)
    d_in, d_aw = engine.block_backward(x.to(dev), clip.visual.transformer.resblocks[0], c["B"], c["L"], cfg.vision.heads,
                                       d_dev, adapter_weight=aw_dev, mix=c["mix"], need_input_grad=want_d_in,
                                       in_place=alias, precision="bf16x3")
    errs = {"d_adapter_w": rel(d_aw, want_daw)}
    if want_d_in:
        assert (d_in.data_ptr() == d_dev.data_ptr()) == alias
        errs["d_in"] = rel(d_in, want_dx)
    else:
        assert d_in is None
    tag = "weight_only" if not want_d_in else ("alias" if alias else "plain")
    print("block bf16x3 adapter", tag, errs)
    PARITY_ERRORS[f"backward_bf16x3.block.adapter.{tag}"] = errs
    assert all(v <= BAR for v in errs.values()), errs


# ---------------------------------------------------------------------------------------------- refusals
def test_short_workspace_is_refused(dev):
    B, H, L = 1, 2, 32
    qkv, d_ctx, _ = VB.attention_case(B, H, L, False)
    q, d = qkv.to(dev), d_ctx.to(dev)
    out = torch.full_like(q, 7.0)
    lib = _lib.load()
    need = lib.aaclip_attention_backward_long_bf16x3_workspace_bytes(B, L, H)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rc = lib.aaclip_attention_backward_long_bf16x3(q.data_ptr(), d.data_ptr(), out.data_ptr(), B, L, H, 0, 1.0,
                                                   ws.data_ptr(), need - 1, None)
    torch.cuda.synchronize()
    assert rc < 0 and b"workspace too small" in lib.aaclip_last_error()
    assert bool((out == 7.0).all())
    rc = lib.aaclip_attention_backward_long_bf16x3(q.data_ptr(), d.data_ptr(), out.data_ptr(), B, L, H, 0, 1.0,
                                                   ws.data_ptr(), need, None)
    torch.cuda.synchronize()
    assert rc == 0 and not bool((out == 7.0).any())


def test_block_refusals(dev, block_models):
    cfg, sd, clip = block_models["tiny"]
    D, H, L = cfg.vision.width, cfg.vision.heads, 33
    block = clip.visual.transformer.resblocks[0]
    x = rnd("bf16x3.refuse.x", (L, D)).to(dev)
    d_out = torch.full_like(x, 7.0)
    with pytest.raises(RuntimeError, match="D must equal 64"):
        engine.block_backward(x, block, 1, L, H + 1, d_out, precision="bf16x3")
    with pytest.raises(ValueError, match="bf16x3"):
        engine.block_backward(x, block, 1, L, H, d_out, precision="bf16")
    lib = _lib.load()
    F = block.mlp.c_fc.weight.shape[0]
    w, refs = engine.pack_block(block, engine.F32, None)
    w3, refs3 = engine.pack_block_split3(block)
    wt3, refs_t = engine.pack_block_split3_transposed(block, None)
    need = lib.aaclip_block_backward_long_bf16x3_workspace_bytes(1, L, D, F)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    d_in = torch.full_like(x, 7.0)
    args = (x.data_ptr(), C.byref(w), C.byref(w3), C.byref(wt3), 0.0, 1, L, D, H, F, engine.ATTN_FULL, d_out.data_ptr(),
            d_in.data_ptr(), None, ws.data_ptr())
    rc = lib.aaclip_block_backward_long_bf16x3(*args, need - 1, None)
    torch.cuda.synchronize()
    assert rc < 0 and b"workspace too small" in lib.aaclip_last_error()
    assert bool((d_in == 7.0).all())
    assert lib.aaclip_block_backward_long_bf16x3(*args[:10], 5, *args[11:], need, None) < 0      # a bad attn_mode
    assert lib.aaclip_block_backward_long_bf16x3(None, *args[1:], need, None) < 0                # a null pointer
    assert bool((d_in == 7.0).all())
    del refs, refs3, refs_t


# ---------------------------------------------------------------------------------------------- the whole model
def adapter_params(model):
    return [m.weight for m in model.image_adapter["layer_adapters"]]


def hip_loss(model, image, mask, anchors):
    """tests/test_gpu_visual_backward.py's composition: the heads of AdaptedCLIP.forward from torch ops on the tap
    streams, then the stage's map + segmentation loss per level, summed -> (loss, [tap streams])"""
    v = model.image_encoder
    loss, taps = 0, autograd.visual_taps(model, image)
    for k, tap in enumerate(taps):
        t = torch.nn.functional.layer_norm(tap[:, 1:, :], (tap.shape[-1],), v.ln_post.weight, v.ln_post.bias, 1e-5)
        seg = torch.nn.functional.normalize(t @ model.image_adapter["seg_proj"][k].weight.t(), dim=-1)
        loss = loss + FU.calculate_seg_loss(FU.calculate_similarity_map(seg, anchors, VB.TAPS_IMAGE), mask)
    return loss, [t.detach().clone() for t in taps]


def oracle_gradients(cfg, sd, ia, image, mask, anchors):
    leaves = {k: v.double() for k, v in ia.items()}
    keys = [f"layer_adapters.{i}.fc.0.weight" for i in range(VB.TAPS_UNTIL)]
    for k in keys:
        leaves[k].requires_grad_(True)
    seg, _ = O.adapted_visual_forward(image, sd, leaves, cfg.vision.heads, VB.TAPS_MIX, VB.TAPS_UNTIL, VB.TAPS_LEVELS,
                                      relu=False, dtype=torch.float64)
    sum(sum(seg_loss_terms(similarity_map(s, anchors, VB.TAPS_IMAGE), mask)) for s in seg).backward()
    return [leaves[k].grad for k in keys]


@pytest.mark.parametrize("precision", ["fp32", "fp16x2"])
def test_visual_taps_gradients(dev, precision):
    cfg, sd, ia, model = VB.build_taps_model(dev, precision)
    image, mask, anchors = VB.taps_inputs()
    g64 = oracle_gradients(cfg, sd, ia, image, mask, anchors)
    args = (model, image.to(dev), mask.float().to(dev), anchors.float().to(dev))
    runs = {}
    for mode in ("fp32", "bf16x3"):
        model.zero_grad(set_to_none=True)
        with autograd.use_backward_precision(mode):
            loss, taps = hip_loss(*args)
            loss.backward()
        runs[mode] = (loss.detach().clone(), taps, [p.grad.clone() for p in adapter_params(model)])
    assert autograd.backward_precision() == "fp32"
    assert torch.equal(runs["fp32"][0], runs["bf16x3"][0])
    for a, b in zip(runs["fp32"][1], runs["bf16x3"][1]):
        assert torch.equal(a, b)
    errs = {"vs_fp64": [rel(g, w) for g, w in zip(runs["bf16x3"][2], g64)],
            "fp32_backward_vs_fp64": [rel(g, w) for g, w in zip(runs["fp32"][2], g64)],
            "vs_fp32_backward": [rel(g, w) for g, w in zip(runs["bf16x3"][2], runs["fp32"][2])]}
    print("visual_taps bf16x3 backward,", precision, "forward:", errs)
    PARITY_ERRORS[f"backward_bf16x3.taps.{precision}"] = errs
    assert any(not torch.equal(a, b) for a, b in zip(runs["fp32"][2], runs["bf16x3"][2]))     # the other arithmetic ran
    assert all(e <= 1e-2 for e in errs["vs_fp64"]), errs


# ---------------------------------------------------------------------------------------------- one stage-2 step
def stage2_model(dev):
    """The reduced model (image 182, L = 170, D = 256) with an IQM branch 256 wide, every stage-2 parameter trainable"""
    from model.adapter import AdaptedCLIP
    cfg = VB.taps_cfg()
    sd, clip = VB.build_clip(cfg, "fp32", 7)
    ia = synth.synth_image_adapter_state_dict(cfg, until=VB.TAPS_UNTIL, levels=len(VB.TAPS_LEVELS), relu=False, seed=7)
    model = AdaptedCLIP(clip, text_adapt_until=1, image_adapt_until=VB.TAPS_UNTIL, levels=VB.TAPS_LEVELS, relu=False,
                        image_adapt_weight=VB.TAPS_MIX, iqm_hidden_size=256, iqm_num_heads=8)
    model.image_adapter.load_state_dict(ia, strict=True)
    isd = synth.synth_iqm_state_dict(cfg, levels=len(VB.TAPS_LEVELS), relu=False, hidden=256, seed=111)
    _, unexpected = model.load_state_dict(isd, strict=False)
    assert not unexpected
    for p in model.parameters():
        p.requires_grad_(False)
    groups = (list(model.image_adapter.parameters()) + list(model.iqm.parameters())
              + list(model.class_query_mlp.parameters()) + list(model.query_adapters.parameters()))
    for p in groups:
        p.requires_grad_(True)
    return model.to(dev).eval()


def test_one_stage2_step(dev):
    import train
    model = stage2_model(dev)
    image, mask, anchors, label = HB.heads_inputs()
    args = (model, image.to(dev), mask.float().to(dev), label.to(dev), anchors.float().to(dev), VB.TAPS_IMAGE)
    runs = {}
    for mode in ("fp32", "bf16x3"):
        model.zero_grad(set_to_none=True)
        with autograd.use_backward_precision(mode):
            loss = train.stage2_loss(*args)
            loss.backward()
        runs[mode] = (loss.detach().clone(), {k: None if p.grad is None else p.grad.clone()
                                              for k, p in model.named_parameters() if p.requires_grad})
    assert torch.isfinite(runs["fp32"][0]) and torch.equal(runs["fp32"][0], runs["bf16x3"][0])
    errs = {}
    for k, g in runs["fp32"][1].items():
        h = runs["bf16x3"][1][k]
        assert (g is None) == (h is None), k
        if g is not None:
            errs[k] = 0.0 if not g.any() and not h.any() else rel(h, g)
    worst = max(errs, key=errs.get)
    layer = {k: e for k, e in errs.items() if "layer_adapters" in k}
    print("stage-2 step, bf16x3 against fp32 backward: worst", worst, errs[worst], "layer adapters", layer)
    PARITY_ERRORS["backward_bf16x3.stage2_step"] = {"worst": errs[worst], "layer_adapters": layer}
    assert layer and any(e > 0 for e in layer.values())             # the other arithmetic ran
    assert all(e <= 1e-2 for e in errs.values()), {k: e for k, e in errs.items() if e > 1e-2}
