"""Shapes, inputs and fp64 references shared by tests/test_head_backward_cpu.py and tests/test_gpu_head_backward.py
(aaclip_tap_head_backward, autograd.visual_heads, train.stage2_text_loss)."""
import functools

import torch
import torch.nn.functional as F

import oracle.aaclip_oracle as O
import visual_backward_cases as VB
from seg_loss_cases import seg_loss_terms, similarity_map
from visual_backward_cases import rnd

NONE, LEAKY = 0, 1                       # AACLIP_ACT_NONE, AACLIP_ACT_LEAKY
BOTH, SEG_ONLY, DET_ONLY = "yes", "no", "det only"
Z_MARGIN = 1e-5

# name -> (B, L, D, E, act, det, d_x wanted, draw).  The inputs are drawn from the case's name and `draw`.  With the
# LeakyReLU the reference's derivative jumps where a projection pre-activation z is 0, so a leaky case must keep every
# |z| of its patch rows above the fp32 error of z (~1e-6 at z rms 1.3, see visual_backward_cases.py): head_case
# asserts |z| > Z_MARGIN in fp64.  `draw` is the first draw of that name for which it holds (min_abs_z_search finds it;
# among 1.4 M values of rms 1.3 one below 1e-5 is the rule, not the exception).
HEAD_CASES = {
    "one_patch": (1, 2, 256, 256, NONE, BOTH, True, 0),                        # one patch per image
    "cls_rows_interleaved": (3, 5, 256, 256, LEAKY, BOTH, True, 0),            # 15 rows, 4 per workgroup; |z| >= 9.1e-5
    "other_widths": (2, 50, 768, 1024, NONE, BOTH, True, 0),
    "production": (2, 170, 1024, 768, NONE, BOTH, True, 0),
    "production_leaky_no_det": (2, 170, 1024, 768, LEAKY, SEG_ONLY, True, 4),            # smallest |z| 1.4e-5
    "production_weights_only": (2, 170, 1024, 768, NONE, BOTH, False, 0),
    "production_det_only": (2, 170, 1024, 768, NONE, DET_ONLY, True, 0),
    "visual_length": (1, 1370, 256, 256, LEAKY, BOTH, True, 45),               # 11 wgrad row chunks; |z| >= 1.2e-5
}


def head_inputs(name, draw=None):
    """-> dict of fp32 CPU tensors: x [B*L, D], ln_w, ln_b [D], proj_w, det_w [E, D], d_seg [B, L-1, E], d_det [B, E]
    (all drawn, whatever parts the case uses)"""
    B, L, D, E, _, _, _, d0 = HEAD_CASES[name]
    tag = f"head.{name}.{d0 if draw is None else draw}."
    return {
        "x": rnd(tag + "x", (B * L, D), 1.5) + 0.3,
        "ln_w": rnd(tag + "ln_w", (D,), 0.1) + 1.0,
        "ln_b": rnd(tag + "ln_b", (D,), 0.05),
        "proj_w": rnd(tag + "proj_w", (E, D), 1.3 * D ** -0.5),
        "det_w": rnd(tag + "det_w", (E, D), 1.3 * D ** -0.5),
        "d_seg": rnd(tag + "d_seg", (B, L - 1, E)),
        "d_det": rnd(tag + "d_det", (B, E)),
    }


def _head_autograd(name, t):
    """fp64 torch autograd of the head: layer_norm, drop the CLS row, project, activation, F.normalize, (patch mean,)
    contracted with d_seg / d_det -> ({d_x, d_proj_w, d_det_w} with None for what the case lacks, smallest |z|)"""
    B, L, D, E, act, det, want_dx, _ = HEAD_CASES[name]
    x = t["x"].double().reshape(B, L, D).requires_grad_(True)
    pw, dw = t["proj_w"].double().requires_grad_(True), t["det_w"].double().requires_grad_(True)
    ln = F.layer_norm(x, (D,), t["ln_w"].double(), t["ln_b"].double(), 1e-5)[:, 1:, :]
    loss, zmin = 0, float("inf")
    parts = []
    if det != DET_ONLY:
        parts.append((pw, t["d_seg"].double(), False))
    if det != SEG_ONLY:
        parts.append((dw, t["d_det"].double(), True))
    for w, d, mean in parts:
        z = ln @ w.t()
        zmin = min(zmin, float(z.detach().abs().min()))
        y = F.normalize(F.leaky_relu(z, 0.01) if act == LEAKY else z, dim=-1)
        loss = loss + ((y.mean(dim=1) if mean else y) * d).sum()
    loss.backward()
    return {"d_x": x.grad.reshape(B * L, D) if want_dx else None,
            "d_proj_w": pw.grad if det != DET_ONLY else None,
            "d_det_w": dw.grad if det != SEG_ONLY else None}, zmin


@functools.lru_cache(maxsize=None)
def head_case(name):
    """-> (inputs, fp64 gradients): computed once, shared, never modified"""
    t = head_inputs(name)
    want, zmin = _head_autograd(name, t)
    if HEAD_CASES[name][4] == LEAKY:
        assert zmin > Z_MARGIN, f"{name}: a pre-activation of {zmin:.2e} sits on the LeakyReLU kink; choose another draw"
    return t, want


def min_abs_z_search(name, draws=range(400)):
    """The first draw of a leaky case whose smallest |z| exceeds Z_MARGIN (how the `draw` column was filled)."""
    for d in draws:
        zmin = _head_autograd(name, head_inputs(name, d))[1]
        if zmin > Z_MARGIN:
            return d, zmin
    raise AssertionError(name)


# ---------------------------------------------------------------------------------------------- whole model
HEADS_LABELS = [0, 1]
HEADS_KEYS = ([f"layer_adapters.{i}.fc.0.weight" for i in range(VB.TAPS_UNTIL)]
              + [f"seg_proj.{k}.fc.weight" for k in range(len(VB.TAPS_LEVELS))] + ["det_proj.fc.weight"])


def build_heads_model(dev, precision, train_adapters=True, train_projections=True):
    """visual_backward_cases.build_taps_model with seg_proj and det_proj trainable as well (or only one of the two
    families)."""
    cfg, sd, ia, model = VB.build_taps_model(dev, precision)
    for p in model.image_adapter["layer_adapters"].parameters():
        p.requires_grad_(train_adapters)
    for part in ("seg_proj", "det_proj"):
        for p in model.image_adapter[part].parameters():
            p.requires_grad_(train_projections)
    return cfg, sd, ia, model


def heads_params(model):
    """name -> parameter, in the order of HEADS_KEYS"""
    ia = model.image_adapter
    ps = [m.weight for m in ia["layer_adapters"]] + [m.weight for m in ia["seg_proj"]] + [ia["det_proj"].weight]
    return dict(zip(HEADS_KEYS, ps))


def heads_inputs():
    """-> (images [B, 3, S, S] fp32, mask [B, 1, S, S] fp64, per-image anchors [B, E, 2] fp64 with unit columns, labels
    [B] int64)"""
    image, mask, _ = VB.taps_inputs()
    t = rnd("heads.anchors", (VB.TAPS_BATCH, 256, 2)).double()
    return image, mask, t / t.norm(dim=1, keepdim=True), torch.tensor(HEADS_LABELS)


def oracle_stage2(dtype):
    """The oracle's forward and the stage-2 text loss written in torch, in `dtype` on the CPU -> (loss, gradients by
    HEADS_KEYS, seg tokens, det token)"""
    cfg, sd, ia, _ = build_heads_model(torch.device("cpu"), "fp32")
    image, mask, anchors, label = heads_inputs()
    leaves = {k: v.to(dtype) for k, v in ia.items()}
    for k in HEADS_KEYS:
        leaves[k].requires_grad_(True)
    seg, det = O.adapted_visual_forward(image, sd, leaves, cfg.vision.heads, VB.TAPS_MIX, VB.TAPS_UNTIL, VB.TAPS_LEVELS,
                                        relu=False, dtype=dtype)
    a = anchors.to(dtype)
    loss = 0.5 * F.cross_entropy(torch.matmul(det.unsqueeze(1), a)[:, 0], label)
    for s in seg:
        loss = loss + 0.6 * 0.5 * sum(seg_loss_terms(similarity_map(s, a, VB.TAPS_IMAGE), mask.to(dtype)))
    loss.backward()
    return loss.item(), {k: leaves[k].grad for k in HEADS_KEYS}, [s.detach() for s in seg], det.detach()


@functools.lru_cache(maxsize=None)
def oracle_stage2_fp64():
    return oracle_stage2(torch.float64)
