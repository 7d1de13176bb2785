"""Backward of the adapted text tower on the GPU (csrc/text_backward.hip, aaclip_hip.autograd.TextTower, train.py).

Bars.  Building blocks and aaclip_block_backward against fp64 torch autograd: 1e-4 relative Frobenius, the project's bar
for fp32 gradients (tests/test_gpu_seg_loss.py).  Whole-model gradients with precision fp32: the yardstick is the
oracle's own fp32 CPU autograd against its fp64 autograd, computed in the same test (e_ref: what the reference's fp32
training delivers); the HIP gradient's error against fp64 may be at most 8 x e_ref (same arithmetic width, another
summation order).  precision fp16x2 (only the saved streams differ): 1e-2 relative Frobenius, the relative part of
BASELINE.json's tolerance.  Train-step losses: 1e-5 relative, the loss bar of tests/test_gpu_seg_loss.py.
Every measured error goes to PARITY_ERRORS."""
import logging
import math
import os

import pytest
import torch

import forward_utils as FU
import oracle.aaclip_oracle as O
import text_backward_cases as TB
from aaclip_hip import _lib, engine, synth
from conftest import PARITY_ERRORS
from model.tokenizer import tokenize
from seg_loss_cases import seg_loss_terms, similarity_map

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.isfinite(a).all()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def rnd(name, shape, std=1.0):
    return synth.randn("tb." + name, shape, std, 23)


# ---------------------------------------------------------------------------------------------- building blocks
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("L", [1, 5, 77, 128])
@pytest.mark.parametrize("B,H", [(1, 1), (3, 4), (2, 12)])
def test_attention_backward(dev, causal, L, B, H):
    D = 64 * H
    qkv = rnd(f"attn.qkv.{B}.{L}.{H}", (B * L, 3 * D))
    qkv[:, :D] *= 0.5                      # q as the block passes it: already scaled
    d_ctx = rnd(f"attn.dctx.{B}.{L}.{H}", (B * L, D))
    x = qkv.double().requires_grad_(True)
    q, k, v = (t.reshape(B, L, H, 64).transpose(1, 2) for t in x.split(D, dim=-1))
    s = q @ k.transpose(-1, -2)
    if causal:
        s = s + O.causal_mask(L, torch.float64)
    ctx = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B * L, D)
    ctx.backward(d_ctx.double())
    got = engine.attention_backward(qkv.to(dev), d_ctx.to(dev), B, L, H, causal)
    e = rel(got, x.grad)
    PARITY_ERRORS[f"text_backward.attention.{'causal' if causal else 'full'}.B{B}.L{L}.H{H}"] = e
    assert e <= 1e-4, e
    if L == 77 and H == 4:                 # dq_scale multiplies the dq columns only
        got2 = engine.attention_backward(qkv.to(dev), d_ctx.to(dev), B, L, H, causal, dq_scale=0.125)
        assert torch.equal(got2[:, D:], got[:, D:])
        assert rel(got2[:, :D], 0.125 * x.grad[:, :D]) <= 1e-4


@pytest.mark.parametrize("rows", [77, 1232, 4929])
@pytest.mark.parametrize("O_,I_", [(768, 768), (256, 768), (256, 256)])
def test_gemm_wgrad(dev, rows, O_, I_):
    dz = rnd(f"wg.dz.{rows}.{O_}", (rows, O_))
    u = rnd(f"wg.u.{rows}.{I_}", (rows, I_))
    want = dz.double().t() @ u.double()
    got = engine.gemm_wgrad(dz.to(dev), u.to(dev))
    e = rel(got, want)
    PARITY_ERRORS[f"text_backward.wgrad.rows{rows}.{O_}x{I_}"] = e
    assert e <= 1e-4, e
    assert torch.equal(got, engine.gemm_wgrad(dz.to(dev), u.to(dev)))


@pytest.mark.parametrize("D", [256, 768])
def test_layernorm_backward(dev, D):
    rows = 131
    x = rnd(f"ln.x.{D}", (rows, D), 2.0) + 0.3
    w = rnd(f"ln.w.{D}", (D,), 0.1) + 1.0
    b = rnd(f"ln.b.{D}", (D,), 0.05)
    dy, dr = rnd(f"ln.dy.{D}", (rows, D)), rnd(f"ln.dr.{D}", (rows, D))
    x64 = x.double().requires_grad_(True)
    O.layer_norm(x64, w.double(), b.double()).backward(dy.double())
    got = engine.layernorm_backward(x.to(dev), w.to(dev), dy.to(dev))
    got_r = engine.layernorm_backward(x.to(dev), w.to(dev), dy.to(dev), dr.to(dev))
    e, e_r = rel(got, x64.grad), rel(got_r, x64.grad + dr.double())
    PARITY_ERRORS[f"text_backward.layernorm.D{D}"] = e
    assert e <= 1e-4 and e_r <= 1e-4, (e, e_r)


@pytest.mark.parametrize("D", [256, 768])
def test_adapter_mix_backward(dev, D):
    rows, mix = 131, 0.1
    u, z, dy = rnd(f"mix.u.{D}", (rows, D), 1.5), rnd(f"mix.z.{D}", (rows, D)), rnd(f"mix.dy.{D}", (rows, D))
    u64, z64 = u.double().requires_grad_(True), z.double().requires_grad_(True)
    a = O.leaky_relu(z64)
    y = mix * a * u64.norm(dim=-1, keepdim=True) / a.norm(dim=-1, keepdim=True) + (1 - mix) * u64
    y.backward(dy.double())
    d_z, d_u = engine.adapter_mix_backward(u.to(dev), z.to(dev), dy.to(dev), mix)
    e_z, e_u = rel(d_z, z64.grad), rel(d_u, u64.grad)
    PARITY_ERRORS[f"text_backward.adapter_mix.D{D}"] = {"d_z": e_z, "d_u": e_u}
    assert e_z <= 1e-4 and e_u <= 1e-4, (e_z, e_u)


class _LN:
    def __init__(self, w, b):
        self.weight, self.bias = w, b


@pytest.mark.parametrize("D", [256, 768])
def test_row_head_backward(dev, D):
    n, T, E = 5, 77, 256 if D == 256 else 768
    x = rnd(f"rh.x.{D}", (n * T, D), 1.5)
    w, b = rnd(f"rh.w.{D}", (D,), 0.1) + 1.0, rnd(f"rh.b.{D}", (D,), 0.05)
    proj = rnd(f"rh.p.{D}", (E, D), D ** -0.5)
    d_out = rnd(f"rh.do.{D}", (n, E))
    tokens = torch.randint(1, 1000, (n, T), generator=torch.Generator().manual_seed(D), dtype=torch.int32)
    eot = [3, 76, 0, 40, 12]
    for i, t in enumerate(eot):
        tokens[i, t] = 49407
    x64, p64 = x.double().requires_grad_(True), proj.double().requires_grad_(True)
    rows = O.layer_norm(x64, w.double(), b.double()).reshape(n, T, D)[torch.arange(n), torch.tensor(eot)]
    O.leaky_relu(rows @ p64.t()).backward(d_out.double())
    ln = _LN(w.to(dev), b.to(dev))
    pd = proj.to(dev)
    d_x, d_w = engine.row_head_backward(x.to(dev), tokens.to(dev), ln, pd, _lib.ACT_LEAKY, d_out.to(dev), n, T, 0)
    e_x, e_w = rel(d_x, x64.grad), rel(d_w, p64.grad)
    PARITY_ERRORS[f"text_backward.row_head.D{D}"] = {"d_x": e_x, "d_proj": e_w}
    assert e_x <= 1e-4 and e_w <= 1e-4, (e_x, e_w)
    picked = torch.tensor([i * T + t for i, t in enumerate(eot)])
    other = torch.ones(n * T, dtype=torch.bool)
    other[picked] = False
    assert not d_x.cpu()[other].any()                      # a scatter into an otherwise zero stream gradient
    _, d_w2 = engine.row_head_backward(x.to(dev), tokens.to(dev), ln, pd, _lib.ACT_LEAKY, d_out.to(dev), n, T, 0,
                                       need_input_grad=False)
    assert torch.equal(d_w, d_w2)


# ---------------------------------------------------------------------------------------------- models
def build_tiny(dev, precision, until=1):
    from model.adapter import AdaptedCLIP
    from model.model import CLIP
    cfg = synth.tiny_cfg()
    sd = synth.synth_clip_state_dict(cfg, seed=7)
    clip = CLIP(cfg.embed_dim,
                dict(image_size=cfg.image_size, layers=cfg.vision.layers, width=cfg.vision.width,
                     patch_size=cfg.patch_size),
                dict(context_length=77, vocab_size=cfg.vocab_size, width=cfg.text.width, heads=cfg.text.heads,
                     layers=cfg.text.layers), precision=precision)
    clip.load_state_dict(sd, strict=True)
    ta = synth.synth_text_adapter_state_dict(cfg, until=until, seed=7)
    model = AdaptedCLIP(clip, text_adapt_until=until, image_adapt_until=2, levels=[2, 3], relu=False)
    model.text_adapter.load_state_dict(ta, strict=True)
    for p in model.parameters():
        p.requires_grad_(False)
    for p in model.text_adapter.parameters():
        p.requires_grad_(True)
    return cfg, sd, ta, clip.to(dev).eval(), model.to(dev).eval()


@pytest.mark.parametrize("case", ["adapter_alias", "adapter", "adapter_no_d_in", "plain", "plain_full_mask"])
def test_block_backward(dev, case):
    cfg, sd, ta, clip, model = build_tiny(dev, "fp32")
    block = clip.transformer.resblocks[1]
    pre = "transformer.resblocks.1."
    adapter = case.startswith("adapter")
    causal = case != "plain_full_mask"
    B, L, D, H, mix = (3, 77, 256, 4, 0.1) if causal else (2, 50, 256, 4, 0.1)
    x = rnd(f"blk.x.{case}", (B * L, D), 1.0)
    d_out = rnd(f"blk.do.{case}", (B * L, D))
    aw = model.text_adapter[0].weight if adapter else None
    sd64 = {k: v.double() for k, v in sd.items() if k.startswith(pre)}
    x64 = x.double().reshape(B, L, D).requires_grad_(True)
    y = O.resblock(x64, sd64, pre, H, O.causal_mask(L, torch.float64) if causal else None)
    a64 = None
    if adapter:
        a64 = ta["0.fc.0.weight"].double().requires_grad_(True)
        y = O.adapter_mix(y, a64, mix)
    y.backward(d_out.double().reshape(B, L, D))
    d_dev = d_out.to(dev)
    d_in, d_aw = engine.block_backward(x.to(dev), block, B, L, H, d_dev, causal=causal, adapter_weight=aw, mix=mix,
                                       need_input_grad=case != "adapter_no_d_in", in_place=case == "adapter_alias")
    errs = {}
    if case == "adapter_no_d_in":
        assert d_in is None
    else:
        if case == "adapter_alias":
            assert d_in.data_ptr() == d_dev.data_ptr()
        errs["d_in"] = rel(d_in, x64.grad.reshape(B * L, D))
    if adapter:
        errs["d_adapter_w"] = rel(d_aw, a64.grad)
    else:
        assert d_aw is None
    PARITY_ERRORS[f"text_backward.block.{case}"] = errs
    assert all(v <= 1e-4 for v in errs.values()), errs


def hip_loss(model, tok_n, tok_a, f, mask, img):
    t = torch.stack([FU._anchor(model.encode_text(tok_n)), FU._anchor(model.encode_text(tok_a))], dim=1)
    t = t.unsqueeze(0).expand(f.shape[0], -1, -1).contiguous()
    return TB.stage1_loss(t, f, mask, img, TB.NORM_WEIGHT, FU.calculate_similarity_map, FU.calculate_seg_loss)


def oracle_grads(tok_n, tok_a, sd, ta, heads, until, f, mask, img, dtype):
    leaves = {k: v.to(dtype).requires_grad_(True) for k, v in ta.items()}
    loss = TB.oracle_loss(tok_n, tok_a, sd, leaves, heads, until, f, mask, img, TB.NORM_WEIGHT, dtype)
    loss.backward()
    return loss.item(), {k: v.grad for k, v in leaves.items()}


def model_gradient_errors(dev, model, sd, ta, heads, until, tok_n, tok_a, f, mask, img, with_ref=True):
    loss64, g64 = oracle_grads(tok_n, tok_a, sd, ta, heads, until, f, mask, img, torch.float64)
    e_ref = None
    if with_ref:
        _, g32 = oracle_grads(tok_n, tok_a, sd, ta, heads, until, f, mask, img, torch.float32)
        e_ref = {k: rel(g32[k], g64[k]) for k in g64}
    model.zero_grad(set_to_none=True)
    loss = hip_loss(model, tok_n.to(dev), tok_a.to(dev), f.float().to(dev), mask.float().to(dev), img)
    loss.backward()
    got = {k: p.grad for k, p in model.text_adapter.state_dict(keep_vars=True).items()}
    assert set(got) == set(g64)
    e_hip = {k: rel(got[k], g64[k]) for k in g64}
    return abs(loss.item() - loss64) / abs(loss64), e_hip, e_ref


def tiny_tokens():
    normal, abnormal = FU.class_sentences("MVTec", "bottle")      # the packaged prompt table serves these without BPE
    return tokenize(normal[:2]), tokenize(abnormal[:2])


def test_tiny_model_gradients_fp32(dev):
    cfg, sd, ta, clip, model = build_tiny(dev, "fp32")
    tok_n, tok_a = tiny_tokens()
    f, mask = TB.patch_inputs()
    e_loss, e_hip, e_ref = model_gradient_errors(dev, model, sd, ta, cfg.text.heads, 1, tok_n, tok_a, f, mask, TB.IMG)
    print("tiny fp32: loss", e_loss, "hip", e_hip, "ref", e_ref)
    PARITY_ERRORS["text_backward.tiny.fp32"] = {"loss_rel": e_loss, "e_hip": e_hip, "e_ref": e_ref}
    assert e_loss <= 1e-5, e_loss
    for k in e_hip:
        assert e_hip[k] <= 8 * e_ref[k], (k, e_hip[k], e_ref[k])
    for p in clip.parameters():
        assert p.grad is None


def test_tiny_model_gradients_fp16x2(dev):
    cfg, sd, ta, clip, model = build_tiny(dev, "fp16x2")
    tok_n, tok_a = tiny_tokens()
    f, mask = TB.patch_inputs()
    e_loss, e_hip, _ = model_gradient_errors(dev, model, sd, ta, cfg.text.heads, 1, tok_n, tok_a, f, mask, TB.IMG,
                                             with_ref=False)
    print("tiny fp16x2: loss", e_loss, "hip", e_hip)
    PARITY_ERRORS["text_backward.tiny.fp16x2"] = {"loss_rel": e_loss, "e_hip": e_hip}
    for k in e_hip:
        assert e_hip[k] <= 1e-2, (k, e_hip[k])


def test_full_size_text_tower_gradients(dev):
    """768 / 12 heads / 12 layers, text_adapt_until = 3, the 16 sentences of one class (1232 token rows)."""
    from model.adapter import AdaptedCLIP
    from model.model import CLIP
    cfg = synth.ClipCfg(image_size=70, vision=synth.TowerCfg(256, 1, 4, 1024))     # the image side is not used
    sd = synth.synth_clip_state_dict(cfg, seed=111)
    ta = synth.synth_text_adapter_state_dict(cfg, until=3, seed=111)
    clip = CLIP(cfg.embed_dim, dict(image_size=70, layers=1, width=256, patch_size=14),
                dict(context_length=77, vocab_size=cfg.vocab_size, width=768, heads=12, layers=12), precision="fp32")
    clip.load_state_dict(sd, strict=True)
    model = AdaptedCLIP(clip, text_adapt_until=3, image_adapt_until=1, levels=[1], relu=False)
    model.text_adapter.load_state_dict(ta, strict=True)
    for p in model.parameters():
        p.requires_grad_(False)
    for p in model.text_adapter.parameters():
        p.requires_grad_(True)
    model = model.to(dev).eval()
    normal, abnormal = FU.class_sentences("MVTec", "bottle")
    tok_n, tok_a = tokenize(normal), tokenize(abnormal)
    assert tok_n.shape[0] + tok_a.shape[0] == 16
    f, mask = TB.patch_inputs(width=768, name="tb.full")
    e_loss, e_hip, e_ref = model_gradient_errors(dev, model, sd, ta, 12, 3, tok_n, tok_a, f, mask, TB.IMG)
    print("full: loss", e_loss, "hip", e_hip, "ref", e_ref)
    PARITY_ERRORS["text_backward.full_text_tower.fp32"] = {"loss_rel": e_loss, "e_hip": e_hip, "e_ref": e_ref}
    assert e_loss <= 1e-5, e_loss
    for k in e_hip:
        assert e_hip[k] <= 8 * e_ref[k], (k, e_hip[k], e_ref[k])


# ---------------------------------------------------------------------------------------------- behaviour
def test_grad_enabled_embedding_is_bit_identical(dev):
    for precision in ("fp32", "fp16x2", "fp16"):
        cfg, sd, ta, clip, model = build_tiny(dev, precision)
        tok = torch.cat(tiny_tokens()).to(dev)
        with torch.no_grad():
            ref = model.encode_text(tok)
        out = model.encode_text(tok)
        assert out.grad_fn is not None and ref.grad_fn is None
        assert torch.equal(out.detach(), ref), precision


def test_two_backward_passes_are_bit_identical(dev):
    cfg, sd, ta, clip, model = build_tiny(dev, "fp32")
    tok_n, tok_a = (t.to(dev) for t in tiny_tokens())
    f, mask = (t.float().to(dev) for t in TB.patch_inputs())
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        hip_loss(model, tok_n, tok_a, f, mask, TB.IMG).backward()
        runs.append([p.grad.clone() for p in model.text_adapter.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_saved_streams_are_freed(dev):
    cfg, sd, ta, clip, model = build_tiny(dev, "fp32")
    tok = torch.cat(tiny_tokens()).to(dev)
    n = tok.shape[0]
    model.encode_text(tok).sum().backward()        # warm the workspace and the weight caches
    model.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    out = model.encode_text(tok)
    streams = cfg.text.layers * n * 77 * cfg.text.width * 4
    assert torch.cuda.memory_allocated(dev) >= base + streams       # held by the graph
    out.sum().backward()
    del out
    model.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(dev) == base


def test_last_adapter_only_keeps_no_streams(dev):
    cfg, sd, ta, clip, model = build_tiny(dev, "fp32")
    tok = torch.cat(tiny_tokens()).to(dev)
    n = tok.shape[0]
    model.encode_text(tok).sum().backward()
    full = [p.grad.clone() for p in model.text_adapter.parameters()]
    model.zero_grad(set_to_none=True)
    model.text_adapter[0].weight.requires_grad_(False)
    model.encode_text(tok).sum().backward()        # warm this path too
    model.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    out = model.encode_text(tok)
    torch.cuda.synchronize()
    unit = n * 77 * cfg.text.width * 4             # one stream buffer; the stream path holds `layers` of them
    assert torch.cuda.max_memory_allocated(dev) - base < cfg.text.layers * unit
    assert torch.cuda.memory_allocated(dev) - base < unit          # only the n EOT rows and the embedding stay
    out.sum().backward()
    assert model.text_adapter[0].weight.grad is None
    assert rel(model.text_adapter[1].weight.grad, full[1]) <= 1e-6


def test_cpu_tensors_still_raise(dev):
    cfg, sd, ta, clip, model = build_tiny(torch.device("cpu"), "fp32")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.encode_text(torch.cat(tiny_tokens()))


# ---------------------------------------------------------------------------------------------- train step
class _Losses(logging.Handler):
    def __init__(self):
        super().__init__()
        self.values = []

    def emit(self, record):
        msg = record.getMessage()
        if msg.startswith("loss: "):
            self.values.append(float(msg[6:]))


def test_train_text_adapter_three_steps(dev, tmp_path):
    import train
    cfg, sd, ta, clip, model = build_tiny(dev, "fp32")
    _, _, _, clip_surgery, _ = build_tiny(dev, "fp32")
    clip_surgery.visual.DAPM_replace(DPAM_layer=3)
    levels = [1, 2, 3]
    image = synth.synth_images(2, cfg.image_size, seed=7)
    mask = TB.patch_inputs()[1].float()
    classes = ["bottle", "cable"]
    loader = [{"image": image, "mask": mask, "class_name": classes}]       # one batch per epoch, two classes
    lr, w_norm = 2e-5, TB.NORM_WEIGHT
    opt = torch.optim.Adam(model.text_adapter.parameters(), lr=lr, betas=(0.5, 0.999))
    logger = logging.getLogger("test_train_text_adapter")
    logger.setLevel(logging.INFO)
    handler = _Losses()
    logger.addHandler(handler)
    try:
        train.train_text_adapter(model, clip_surgery, w_norm, loader, opt, dev, 0, str(tmp_path), 3, "MVTec",
                                 cfg.image_size, logger, levels=levels)
    finally:
        logger.removeHandler(handler)
    assert len(handler.values) == 3
    # fp64 oracle loop on the same frozen patch features (data: the last tap level is the one that reaches backward)
    f = train.stage1_patch_features(model, clip_surgery, image.to(dev), levels)[-1].double().cpu()
    leaves = {k: v.double().requires_grad_(True) for k, v in ta.items()}
    opt64 = torch.optim.Adam(list(leaves.values()), lr=lr, betas=(0.5, 0.999))
    want = []
    for _ in range(3):
        cols = {}
        for c in classes:
            normal, abnormal = FU.class_sentences("MVTec", c)
            en = O.adapted_encode_text(tokenize(normal), sd, leaves, cfg.text.heads, text_adapt_until=1,
                                       dtype=torch.float64)
            ea = O.adapted_encode_text(tokenize(abnormal), sd, leaves, cfg.text.heads, text_adapt_until=1,
                                       dtype=torch.float64)
            cols[c] = TB.anchors(en, ea)
        t = torch.stack([cols[c] for c in classes], dim=0)
        loss = TB.stage1_loss(t, f, mask.double(), cfg.image_size, w_norm, similarity_map,
                              lambda p, m: sum(seg_loss_terms(p, m)))
        opt64.zero_grad()
        loss.backward()
        opt64.step()
        want.append(loss.item())
    errs = [abs(a - b) / abs(b) for a, b in zip(handler.values, want)]
    print("train losses", handler.values, want, errs)
    PARITY_ERRORS["text_backward.train_step_loss_rel"] = errs
    # the optimizer steps must be visible in the HIP forward (a stale weight copy would leave its losses constant):
    # every step moves the loss by far more than the bar, on both sides
    for k in range(2):
        assert abs(want[k + 1] - want[k]) / want[k] > 1e-3, want
        assert abs(handler.values[k + 1] - handler.values[k]) / handler.values[k] > 1e-3, handler.values
    assert max(errs) <= 1e-5, errs
    # and the trained weights are the oracle's.  Adam's early steps are ~lr * sign(g) per element, so an element only
    # steps differently where |g| is below the gradient's fp32 error (~3e-6 of its rms, measured above): a fraction
    # ~0.8 * 3e-6 of the elements, each off by at most 2 of ~3 lr -> ~1e-3 relative Frobenius of the update; bar 0.05
    for k, p in model.text_adapter.state_dict().items():
        moved = (p.detach().cpu().double() - ta[k].double()).abs()
        assert moved.max() > lr, (k, float(moved.max()))
        e_w = rel(p.detach().cpu().double() - ta[k].double(), leaves[k].detach() - ta[k].double())
        print("trained weight update error", k, e_w)
        PARITY_ERRORS[f"text_backward.train_step_update_rel.{k}"] = e_w
        assert e_w <= 0.05, (k, e_w)
    ck = torch.load(os.path.join(str(tmp_path), "text_adapter.pth"), map_location="cpu")
    assert set(ck) == {"epoch", "text_adapter", "text_optimizer"} and ck["epoch"] == 3
    _, _, _, _, fresh = build_tiny(dev, "fp32")
    fresh.text_adapter.load_state_dict(ck["text_adapter"], strict=True)
    for a, b in zip(fresh.text_adapter.parameters(), model.text_adapter.parameters()):
        assert torch.equal(a, b)
    opt2 = torch.optim.Adam(fresh.text_adapter.parameters(), lr=lr, betas=(0.5, 0.999))
    opt2.load_state_dict(ck["text_optimizer"])
    assert not math.isnan(sum(handler.values))
