"""The tap / det head backward on the GPU: aaclip_tap_head_backward against fp64 torch autograd, autograd.visual_heads
(forward identity, whole-model gradients, partial training, memory) and train.stage2_text_loss.

Bars, the project's own (tests/test_gpu_visual_backward.py).  The entry point against fp64 torch autograd: 1e-4 relative
Frobenius on each output.  Whole-model gradients with precision fp32: at most 8 x e_ref, e_ref being the oracle's own
fp32 CPU autograd against its fp64 autograd, computed in the same test.  precision fp16x2: 1e-2.
Every measured error goes to PARITY_ERRORS under head_backward.*"""
import pytest
import torch

import head_backward_cases as HB
import train
import visual_backward_cases as VB
from aaclip_hip import autograd, engine
from conftest import PARITY_ERRORS
from visual_backward_cases import rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


class _Ln:
    def __init__(self, w, b):
        self.weight, self.bias = w, b


def run_head(dev, name):
    """-> (d_x, d_proj_w, d_det_w) of engine.tap_head_backward on the case's inputs"""
    B, L, D, E, act, det, want_dx, _ = HB.HEAD_CASES[name]
    t = {k: v.to(dev) for k, v in HB.head_case(name)[0].items()}
    seg, with_det = det != HB.DET_ONLY, det != HB.SEG_ONLY
    return engine.tap_head_backward(t["x"], _Ln(t["ln_w"], t["ln_b"]), t["proj_w"] if seg else None, act,
                                    t["d_seg"] if seg else None, det_weight=t["det_w"] if with_det else None,
                                    d_det=t["d_det"] if with_det else None, need_input_grad=want_dx)


# ---------------------------------------------------------------------------------------------- the entry point
@pytest.mark.parametrize("name", list(HB.HEAD_CASES))
def test_tap_head_backward(dev, name):
    B, L, D, E, act, det, want_dx, _ = HB.HEAD_CASES[name]
    want = HB.head_case(name)[1]
    got = dict(zip(("d_x", "d_proj_w", "d_det_w"), run_head(dev, name)))
    errs = {}
    for k, w in want.items():
        if w is None:
            assert got[k] is None, k
        else:
            assert torch.isfinite(got[k]).all(), k
            errs[k] = rel(got[k], w)
    print("tap_head_backward", name, errs)
    PARITY_ERRORS[f"head_backward.entry.{name}"] = errs
    if want_dx:
        assert not got["d_x"].reshape(B, L, D)[:, 0, :].any()          # CLS rows: exact zeros
    assert errs and all(v <= 1e-4 for v in errs.values()), errs


def test_two_calls_are_bit_identical(dev):
    a, b = run_head(dev, "production"), run_head(dev, "production")
    for u, v in zip(a, b):
        assert u is not None and torch.equal(u, v)


# ---------------------------------------------------------------------------------------------- visual_heads
def test_forward_is_that_of_the_model(dev):
    for precision in ("fp32", "fp16x2"):
        cfg, sd, ia, model = HB.build_heads_model(dev, precision)
        image = HB.heads_inputs()[0].to(dev)
        with torch.no_grad():
            ref_seg, ref_det, _ = model(image)
        seg, det = autograd.visual_heads(model, image)
        assert len(seg) == len(ref_seg) == len(VB.TAPS_LEVELS)
        for s, r in zip(seg, ref_seg):
            assert s.grad_fn is not None and torch.equal(s.detach(), r), precision
        assert det.grad_fn is not None and torch.equal(det.detach(), ref_det), precision
        for p in model.parameters():
            p.requires_grad_(False)
        seg, det = autograd.visual_heads(model, image)                  # nothing trains: no graph, the same bits
        assert det.grad_fn is None and all(s.grad_fn is None for s in seg)
        assert torch.equal(det, ref_det) and all(torch.equal(s, r) for s, r in zip(seg, ref_seg))


def hip_gradients(dev, model):
    """One stage2_text_loss step -> (loss, gradients by HB.HEADS_KEYS, None where a parameter got none)"""
    image, mask, anchors, label = HB.heads_inputs()
    model.zero_grad(set_to_none=True)
    loss = train.stage2_text_loss(model, image.to(dev), mask.float().to(dev), label.to(dev), anchors.float().to(dev),
                                  VB.TAPS_IMAGE)
    loss.backward()
    return loss.item(), {k: None if p.grad is None else p.grad.clone() for k, p in HB.heads_params(model).items()}


def gradient_errors(dev, precision):
    cfg, sd, ia, model = HB.build_heads_model(dev, precision)
    loss64, g64, seg64, det64 = HB.oracle_stage2_fp64()
    loss, g = hip_gradients(dev, model)
    ours = list(HB.heads_params(model).values())
    for p in model.parameters():
        assert p.grad is None or any(p is q for q in ours)      # nothing outside image_adapter receives a gradient
    return abs(loss - loss64) / abs(loss64), {k: rel(g[k], g64[k]) for k in HB.HEADS_KEYS}


def test_stage2_gradients_fp32(dev):
    e_loss, e_hip = gradient_errors(dev, "fp32")
    _, g32, _, _ = HB.oracle_stage2(torch.float32)
    g64 = HB.oracle_stage2_fp64()[1]
    e_ref = {k: rel(g32[k], g64[k]) for k in HB.HEADS_KEYS}
    print("stage2 fp32: loss", e_loss, "hip", e_hip, "ref", e_ref)
    PARITY_ERRORS["head_backward.stage2.fp32"] = {"loss_rel": e_loss, "e_hip": e_hip, "e_ref": e_ref}
    for k in HB.HEADS_KEYS:
        assert e_hip[k] <= 8 * e_ref[k], (k, e_hip, e_ref)


def test_stage2_gradients_fp16x2(dev):
    e_loss, e_hip = gradient_errors(dev, "fp16x2")
    print("stage2 fp16x2: loss", e_loss, "hip", e_hip)
    PARITY_ERRORS["head_backward.stage2.fp16x2"] = {"loss_rel": e_loss, "e_hip": e_hip}
    for k in HB.HEADS_KEYS:
        assert e_hip[k] <= 1e-2, (k, e_hip)


def test_partial_training(dev):
    _, full = hip_gradients(dev, HB.build_heads_model(dev, "fp32")[3])
    adapters = [k for k in HB.HEADS_KEYS if k.startswith("layer_adapters")]
    projections = [k for k in HB.HEADS_KEYS if not k.startswith("layer_adapters")]
    # only seg_proj and det_proj: the taps carry no graph, the tower is not revisited
    model = HB.build_heads_model(dev, "fp32", train_adapters=False)[3]
    image = HB.heads_inputs()[0].to(dev)
    assert all(t.grad_fn is None for t in autograd.visual_taps(model, image))
    _, part = hip_gradients(dev, model)
    errs = {k: rel(part[k], full[k]) for k in projections}
    assert all(part[k] is None for k in adapters)
    # only the layer adapters
    _, part = hip_gradients(dev, HB.build_heads_model(dev, "fp32", train_projections=False)[3])
    errs.update({k: rel(part[k], full[k]) for k in adapters})
    assert all(part[k] is None for k in projections)
    print("partial training", errs)
    PARITY_ERRORS["head_backward.partial_training"] = errs
    assert all(v <= 1e-6 for v in errs.values()), errs


def test_saved_tensors_are_freed(dev):
    cfg, sd, ia, model = HB.build_heads_model(dev, "fp32")
    image = HB.heads_inputs()[0].to(dev)

    def step():
        seg, det = autograd.visual_heads(model, image)
        (sum(s.sum() for s in seg) + det.sum()).backward()

    step()                                          # warm the workspace and the weight caches
    model.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    seg, det = autograd.visual_heads(model, image)
    assert torch.cuda.memory_allocated(dev) > base
    (sum(s.sum() for s in seg) + det.sum()).backward()
    del seg, det
    model.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(dev) == base


def test_cpu_tensors_still_raise(dev):
    model = HB.build_heads_model(torch.device("cpu"), "fp32")[3]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        autograd.visual_heads(model, HB.heads_inputs()[0])
