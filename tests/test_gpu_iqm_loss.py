"""The IQM map term of the stage-2 loss on the GPU: aaclip_iqm_map_train and its backward against the fp64 restatement
of reference train.py:173-212 (tests/iqm_loss_cases.py), autograd.iqm_map_train and train.stage2_loss.

Bars.  Forward, both channels and the patch grid against fp64: 2e-6 abs + 1e-6 rel, the bar test_iqm_map_vs_oracle uses;
channel 1 is bit-identical to engine.iqm_map with the one level.  Backward against fp64 autograd: 1e-4 relative
Frobenius on each output, the project's bar for every training entry point (the reference in fp32 on the CPU stays
within 2.5e-5: tests/test_iqm_loss_cpu.py).  Whole model: loss 1e-5 relative; gradients with precision fp32 at most
8 x e_ref, e_ref being the oracle's own fp32 CPU autograd against its fp64 autograd, computed in the same test; precision
fp16x2: 1e-2 (the bars of tests/test_gpu_head_backward.py).
Every measured error goes to PARITY_ERRORS under iqm_loss.*"""
import pytest
import torch

import head_backward_cases as HB
import iqm_loss_cases as IC
import train
import visual_backward_cases as VB
from aaclip_hip import _lib, autograd, engine
from conftest import PARITY_ERRORS
from visual_backward_cases import rel

pytestmark = pytest.mark.gpu
NAMES = list(IC.IQM_CASES)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def close(a, b, atol, rtol, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.isfinite(a).all(), what
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} outside {atol}+{rtol}|ref|, max err {err.max():.3e}"
    return float(err.max())


def on(dev, name):
    t = IC.iqm_case(name)[0]
    return t["seg"].to(dev), t["queries"].to(dev), t["d_preds"].to(dev)


# ---------------------------------------------------------------------------------------------- the entry points
@pytest.mark.parametrize("name", NAMES)
def test_forward(dev, name):
    B, g, S, E, _, _ = IC.IQM_CASES[name]
    want = IC.iqm_case(name)[1]
    seg, q, _ = on(dev, name)
    out, grid = engine.iqm_map_train(seg, q, S)
    assert out.shape == (B, 2, S, S) and grid.shape == (B, g * g)
    errs = {"normal": close(out[:, 0], want["map"][:, 0], 2e-6, 1e-6, "channel 0"),
            "abnormal": close(out[:, 1], want["map"][:, 1], 2e-6, 1e-6, "channel 1"),
            "grid": close(grid, want["p"], 2e-6, 1e-6, "grid")}
    print("iqm_map_train", name, errs)
    PARITY_ERRORS[f"iqm_loss.forward.{name}"] = errs
    assert torch.equal(out[:, 1], engine.iqm_map([seg], q, S)), "channel 1 is engine.iqm_map of the one level"


@pytest.mark.parametrize("name", NAMES)
def test_backward(dev, name):
    want = IC.iqm_case(name)[1]
    seg, q, d_preds = on(dev, name)
    grid = engine.iqm_map_train(seg, q, d_preds.shape[-1])[1]
    d_seg, d_q = engine.iqm_map_train_backward(seg, q, grid, d_preds)
    errs = {"d_seg": rel(d_seg, want["d_seg"]), "d_queries": rel(d_q, want["d_queries"])}
    print("iqm_map_train_backward", name, errs)
    PARITY_ERRORS[f"iqm_loss.backward.{name}"] = errs
    assert all(v <= 1e-4 for v in errs.values()), errs
    only_seg = engine.iqm_map_train_backward(seg, q, grid, d_preds, need_seg=True, need_queries=False)
    only_q = engine.iqm_map_train_backward(seg, q, grid, d_preds, need_seg=False, need_queries=True)
    assert only_seg[1] is None and torch.equal(only_seg[0], d_seg)
    assert only_q[0] is None and torch.equal(only_q[1], d_q)


def test_two_calls_are_bit_identical(dev):
    for name in ("production", "largest_grid"):
        seg, q, d_preds = on(dev, name)
        S = d_preds.shape[-1]
        (o1, g1), (o2, g2) = engine.iqm_map_train(seg, q, S), engine.iqm_map_train(seg, q, S)
        assert torch.equal(o1, o2) and torch.equal(g1, g2)
        a, b = engine.iqm_map_train_backward(seg, q, g1, d_preds), engine.iqm_map_train_backward(seg, q, g1, d_preds)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_degenerate_row(dev):
    """One seg row of zeros: the cosine's clamp is active there, its denominator a constant.  Everything stays finite,
    and no other row of d_seg changes by a bit."""
    seg, q, d_preds = on(dev, "g5")
    S = d_preds.shape[-1]
    row = (1, 7)
    zeroed = seg.clone()
    zeroed[row] = 0
    out, grid = engine.iqm_map_train(zeroed, q, S)
    d_seg, d_q = engine.iqm_map_train_backward(zeroed, q, grid, d_preds)
    for t in (out, grid, d_seg, d_q):
        assert torch.isfinite(t).all()
    assert grid[row] == 0.5                                                # both cosines are 0
    ref = engine.iqm_map_train_backward(seg, q, engine.iqm_map_train(seg, q, S)[1], d_preds)[0]
    keep = torch.ones(seg.shape[:2], dtype=torch.bool, device=dev)
    keep[row] = False
    assert torch.equal(d_seg[keep], ref[keep])
    assert not torch.equal(d_seg[row], ref[row])


def test_rejections_leave_outputs_untouched(dev):
    lib = _lib.load()
    B, g, S, E = 2, 5, 33, 256
    seg, q, d_preds = on(dev, "g5")
    grid = engine.iqm_map_train(seg, q, S)[1]
    need = lib.aaclip_iqm_map_train_backward_workspace_bytes(B, g, E, S)
    # the largest rejected shape (g = 41, S = 2049) touches nothing, so these buffers only have to hold the valid one
    out = torch.full((B, 2, S, S), 1234.5, device=dev)
    grid_out = torch.full((B, g * g), 1234.5, device=dev)
    d_seg, d_q = torch.full_like(seg, 1234.5), torch.full_like(q, 1234.5)
    ws = torch.full((need,), 0xAB, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def fwd(seg_p=seg.data_ptr(), g=g, E=E, S=S):
        return lib.aaclip_iqm_map_train(seg_p, q.data_ptr(), grid_out.data_ptr(), out.data_ptr(), B, g, E, S, stream)

    def bwd(seg_p=seg.data_ptr(), ds=d_seg.data_ptr(), dq=d_q.data_ptr(), g=g, E=E, S=S, ws_bytes=need):
        return lib.aaclip_iqm_map_train_backward(seg_p, q.data_ptr(), grid.data_ptr(), d_preds.data_ptr(), ds, dq, B, g,
                                                 E, S, ws.data_ptr(), ws_bytes, stream)

    cases = {"E = 100": dict(E=100), "g = 41": dict(g=41), "S = 2049": dict(S=2049),
             "misaligned": dict(seg_p=seg.data_ptr() + 4)}
    for what, kw in cases.items():
        for call in (fwd, bwd):
            assert call(**kw) < 0 and lib.aaclip_last_error(), what
    assert bwd(ds=None, dq=None) < 0 and b"nothing to compute" in lib.aaclip_last_error()
    assert bwd(ws_bytes=need - 1) < 0 and b"workspace too small" in lib.aaclip_last_error()
    torch.cuda.synchronize()
    for t in (out, grid_out, d_seg, d_q):
        assert (t == 1234.5).all()
    assert (ws == 0xAB).all()
    assert fwd() == 0 and bwd() == 0                                       # the same arguments, valid: they run
    torch.cuda.synchronize()
    assert torch.equal(grid_out, grid) and not (d_seg == 1234.5).any() and not (d_q == 1234.5).any()


# ---------------------------------------------------------------------------------------------- autograd
def test_autograd_function(dev):
    want = IC.iqm_case("g5")[1]
    seg, q, d_preds = on(dev, "g5")
    S = d_preds.shape[-1]
    with torch.no_grad():
        plain = autograd.iqm_map_train(seg, q, S)
    assert plain.grad_fn is None and torch.equal(plain, engine.iqm_map_train(seg, q, S)[0])
    full = engine.iqm_map_train_backward(seg, q, engine.iqm_map_train(seg, q, S)[1], d_preds)
    for need_seg, need_q in ((True, True), (True, False), (False, True)):
        s, qq = seg.clone().requires_grad_(need_seg), q.clone().requires_grad_(need_q)
        out = autograd.iqm_map_train(s, qq, S)
        assert out.grad_fn is not None and torch.equal(out.detach(), plain)
        out.backward(d_preds)
        assert (s.grad is not None) == need_seg and (qq.grad is not None) == need_q
        if need_seg:
            assert torch.equal(s.grad, full[0])
        if need_q:
            assert torch.equal(qq.grad, full[1])
    assert rel(full[0], want["d_seg"]) <= 1e-4


# ---------------------------------------------------------------------------------------------- whole model
def hip_step(dev, model):
    """One train.stage2_loss step -> (loss, gradients by HB.HEADS_KEYS + "queries")"""
    image, mask, anchors, label = HB.heads_inputs()
    q = IC.stage2_queries().to(dev).requires_grad_(True)
    model.zero_grad(set_to_none=True)
    loss = train.stage2_loss(model, image.to(dev), mask.float().to(dev), label.to(dev), anchors.float().to(dev),
                             VB.TAPS_IMAGE, q)
    loss.backward()
    grads = {k: p.grad.clone() for k, p in HB.heads_params(model).items()}
    grads["queries"] = q.grad.clone()
    return loss.item(), grads


def gradient_errors(dev, precision):
    model = HB.build_heads_model(dev, precision)[3]
    loss64, _, g64, dq64 = IC.oracle_stage2_iqm_fp64()
    loss, g = hip_step(dev, model)
    want = dict(g64, queries=dq64)
    return abs(loss - loss64) / abs(loss64), {k: rel(g[k], want[k]) for k in want}


def test_stage2_loss_fp32(dev):
    e_loss, e_hip = gradient_errors(dev, "fp32")
    _, _, g32, dq32 = IC.oracle_stage2_iqm(torch.float32)
    _, _, g64, dq64 = IC.oracle_stage2_iqm_fp64()
    e_ref = {k: rel(g32[k], g64[k]) for k in HB.HEADS_KEYS}
    e_ref["queries"] = rel(dq32, dq64)
    print("stage2_loss fp32: loss", e_loss, "hip", e_hip, "ref", e_ref)
    PARITY_ERRORS["iqm_loss.stage2.fp32"] = {"loss_rel": e_loss, "e_hip": e_hip, "e_ref": e_ref}
    assert e_loss <= 1e-5, e_loss
    for k in e_ref:
        assert e_hip[k] <= 8 * e_ref[k], (k, e_hip, e_ref)


def test_stage2_loss_fp16x2(dev):
    e_loss, e_hip = gradient_errors(dev, "fp16x2")
    print("stage2_loss fp16x2: loss", e_loss, "hip", e_hip)
    PARITY_ERRORS["iqm_loss.stage2.fp16x2"] = {"loss_rel": e_loss, "e_hip": e_hip}
    assert e_loss <= 1e-5, e_loss
    for k, v in e_hip.items():
        assert v <= 1e-2, (k, e_hip)


def test_iqm_terms_are_the_difference(dev):
    """stage2_loss - stage2_text_loss = the IQM terms computed alone on the model's seg tokens, and those match the
    oracle's share."""
    model = HB.build_heads_model(dev, "fp32")[3]
    image, mask, anchors, label = HB.heads_inputs()
    args = (model, image.to(dev), mask.float().to(dev), label.to(dev), anchors.float().to(dev), VB.TAPS_IMAGE)
    q = IC.stage2_queries().to(dev)
    with torch.no_grad():
        text = train.stage2_text_loss(*args)
        both = train.stage2_loss(*args, q)
        seg_tokens = model(args[1])[0]
        alone = sum(train.iqm_map_loss(s, q, args[2], VB.TAPS_IMAGE) for s in seg_tokens)
    want = IC.oracle_stage2_iqm_fp64()[1]
    errs = {"difference_vs_alone": abs(float(both - text) - float(alone)) / float(alone),
            "alone_vs_oracle": abs(float(alone) - want) / want}
    print("iqm terms", float(alone), errs)
    PARITY_ERRORS["iqm_loss.stage2.iqm_terms"] = errs
    # both - text is a difference of fp32 sums about (both / alone) times larger than the terms: two roundings of them
    assert errs["difference_vs_alone"] <= 4 * 2.0 ** -24 * float(both) / float(alone), errs
    assert errs["alone_vs_oracle"] <= 1e-5, errs


def test_cpu_tensors_still_raise(dev):
    t = IC.iqm_case("g5")[0]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        autograd.iqm_map_train(t["seg"], t["queries"], 33)
