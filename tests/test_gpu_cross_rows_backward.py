"""aaclip_cross_rows_backward on the GPU against fp64 torch autograd, autograd.cross_rows (forward identity, folding
check against the reference's own cross-attention) and autograd.iqm_visual_rows on the reduced model.

Bars, the project's own: the entry point against fp64 autograd, 1e-4 relative Frobenius on each output (the cases stay
within 2.5e-5 in fp32 CPU autograd: tests/test_cross_rows_backward_cpu.py).  Whole-model gradients with precision fp32:
at most 8 x e_ref, e_ref being the restated oracle's own fp32 CPU autograd against its fp64 autograd, computed in the
same test (the rule of tests/test_gpu_head_backward.py).  Every measured error goes to PARITY_ERRORS under
cross_rows_backward.*"""
import functools

import pytest
import torch

import cross_rows_backward_cases as CB
import visual_backward_cases as VB
from aaclip_hip import autograd, engine, synth
from conftest import PARITY_ERRORS
from cross_rows_backward_cases import rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def run_case(dev, name, act=None, base=True):
    """-> {d_qt, d_x} of engine.cross_rows_backward on the case's inputs (act: override the case's activation;
    base=False: overwrite instead of accumulating)"""
    c = CB.CASES[name]
    t = {k: v.to(dev) for k, v in CB.case(name)[0].items()}
    outs = c.get("outs", "both")
    d_x = t["base"].clone() if c.get("accumulate") and base else None
    d_qt, d_x = engine.cross_rows_backward(t["qt"], t["x"], t["d_out"], c["B"], c["R"], c["Lk"], c.get("code", CB.F32),
                                           act=c.get("act", CB.NONE) if act is None else act, need_qt=outs != "d_x",
                                           need_x=outs != "d_qt", d_x=d_x)
    return {"d_qt": d_qt, "d_x": d_x}


# ---------------------------------------------------------------------------------------------- the entry point
@pytest.mark.parametrize("name", list(CB.CASES))
def test_against_fp64(dev, name):
    want = CB.case(name)[1]
    got = run_case(dev, name)
    errs = {}
    for k, w in want.items():
        if w is None:
            assert got[k] is None, k
        elif float(w.norm()) == 0:
            assert not got[k].any(), k                      # one key: ds = 0 and d_qt = 0 exactly
            errs[k] = 0.0
        else:
            errs[k] = rel(got[k], w)
    print("cross_rows_backward", name, errs)
    PARITY_ERRORS[f"cross_rows_backward.{name}"] = errs
    assert errs and all(v <= 1e-4 for v in errs.values()), errs


@pytest.mark.parametrize("name", ["production", "ragged_tiles", "fp16_rows"])
def test_two_calls_are_bit_identical(dev, name):
    a, b = run_case(dev, name), run_case(dev, name)
    for k in ("d_qt", "d_x"):
        assert torch.equal(a[k], b[k]), k


def test_accumulate_adds_onto_the_buffer(dev):
    base = CB.case("accumulate")[0]["base"].to(dev)
    acc, plain = run_case(dev, "accumulate"), run_case(dev, "accumulate", base=False)
    assert torch.equal(acc["d_qt"], plain["d_qt"])
    want = base.double() + plain["d_x"].double()                    # exact in fp64: the one rounding is the kernel's
    ulp = torch.finfo(torch.float32).eps * want.abs().clamp_min(torch.finfo(torch.float32).tiny)
    assert ((acc["d_x"].double() - want).abs() <= ulp).all()
    assert not torch.equal(acc["d_x"], plain["d_x"])


@pytest.mark.parametrize("name", ["leaky", "relu"])
def test_activation_slope(dev, name):
    act = CB.CASES[name]["act"]
    x = CB.case(name)[0]["x"].to(dev)
    with_act, plain = run_case(dev, name), run_case(dev, name, act=CB.NONE)
    assert torch.equal(with_act["d_qt"], plain["d_qt"])
    assert torch.equal(with_act["d_x"], plain["d_x"] * CB.slope_mask(x, act))
    assert not torch.equal(with_act["d_x"], plain["d_x"])


# ---------------------------------------------------------------------------------------------- autograd.cross_rows
def test_autograd_cross_rows(dev):
    for name in ("ragged_tiles", "fp16_rows"):
        c = CB.CASES[name]
        t = {k: v.to(dev) for k, v in CB.case(name)[0].items()}
        B, R, Lk, code = c["B"], c["R"], c["Lk"], c.get("code", CB.F32)
        qt, x = t["qt"].clone().requires_grad_(True), t["x"].clone().requires_grad_(True)
        out = autograd.cross_rows(qt, x, B, R, Lk)
        assert out.grad_fn is not None and torch.equal(out.detach(), engine.cross_rows(t["qt"], t["x"], B, R, Lk, code))
        g_qt, g_x = torch.autograd.grad(out, (qt, x), t["d_out"])
        d_qt, d_x = engine.cross_rows_backward(t["qt"], t["x"], t["d_out"], B, R, Lk, code)
        assert torch.equal(g_qt, d_qt) and g_x.dtype == x.dtype and torch.equal(g_x, d_x.to(x.dtype))
        out = autograd.cross_rows(qt, t["x"], B, R, Lk)                 # only qt: d_x is not computed
        (g_qt,) = torch.autograd.grad(out, (qt,), t["d_out"])
        assert torch.equal(g_qt, d_qt)


def test_folded_route_equals_the_reference_cross_attention(dev):
    """The reference's cross-attention (visual_feature_proj, key / value Linear, per-head softmax) in fp64 against the
    folded route: the query-side products as differentiable torch matmuls around autograd.cross_rows."""
    B, nq, H, Lk, h = (CB.FOLD[k] for k in ("B", "nq", "H", "Lk", "h"))
    hd, R = h // H, nq * H
    ctx64, dx64, dwk64, dbk64 = CB.fold_reference()
    assert float(dbk64.norm()) <= 1e-12 * float(dwk64.norm())        # the key bias is softmax-invariant
    t = {k: v.to(dev) for k, v in CB.fold_inputs().items()}
    x = t["x"].clone().requires_grad_(True)
    q4 = t["q"].view(B, nq, H, hd)
    qt = torch.einsum("bnhd,hdk->bnhk", q4, t["Wk"].view(H, hd, h)) @ t["P"] / hd ** 0.5
    ebar = autograd.cross_rows(qt.reshape(B * R, h).contiguous(), x.view(B * Lk, h), B, R, Lk).view(B, nq, H, h)
    e2 = ebar @ t["P"].t() + t["pb"]
    ctx = (torch.einsum("bnhk,hdk->bnhd", e2, t["Wv"].view(H, hd, h)) + t["bv"].view(H, hd)).reshape(B, nq, h)
    ctx.backward(t["d_ctx"])
    errs = {"ctx": rel(ctx, ctx64), "d_x": rel(x.grad, dx64)}
    print("cross_rows_backward fold", errs)
    PARITY_ERRORS["cross_rows_backward.fold"] = errs
    assert errs["d_x"] <= 1e-4 and errs["ctx"] <= 1e-4, errs


# ---------------------------------------------------------------------------------------------- iqm_visual_rows
Z_MARGIN = 2e-6     # fp32 pre-activations of rms 0.7 are off by ~1e-7: below this a LeakyReLU slope may flip


@functools.lru_cache(maxsize=None)
def build_model(dev, relu):
    """The reduced model at image size 182 (L = 170, D = 256, h = 768) with seeded query adapters; with the LeakyReLU
    the first draw whose patch-row pre-activations all clear Z_MARGIN in fp64 -> (model, image, taps, draw)"""
    from model.adapter import AdaptedCLIP
    cfg = VB.taps_cfg()
    sd, clip = VB.build_clip(cfg, "fp32", 7)
    ia = synth.synth_image_adapter_state_dict(cfg, until=VB.TAPS_UNTIL, levels=len(VB.TAPS_LEVELS), relu=relu, seed=7)
    model = AdaptedCLIP(clip, text_adapt_until=1, image_adapt_until=VB.TAPS_UNTIL, levels=VB.TAPS_LEVELS, relu=relu,
                        image_adapt_weight=VB.TAPS_MIX)
    model.image_adapter.load_state_dict(ia, strict=True)
    for p in model.parameters():
        p.requires_grad_(False)
    model = model.to(dev).eval()
    image = VB.taps_inputs()[0].to(dev)
    taps = [t.detach() for t in autograd.visual_taps(model, image)]
    ln = model.image_encoder.ln_post
    h, D = model.iqm_hidden_size, taps[0].shape[-1]
    for draw in range(64):
        ws = [CB.rnd(f"qa.{k}.{draw}", (h, D), (2.0 / (h + D)) ** 0.5) for k in range(len(taps))]
        zmin = CB.visual_rows_oracle(taps, ws, ln.weight, ln.bias, relu, torch.zeros(()), torch.float64)[3]
        if not relu or zmin > Z_MARGIN:
            break
    else:
        raise AssertionError("no draw clears the LeakyReLU kink")
    with torch.no_grad():
        for qa, w in zip(model.query_adapters, ws):
            qa.weight.copy_(w)
    for qa in model.query_adapters:
        qa.weight.requires_grad_(True)
    return model, image, taps, draw


def d_rows_of(rows):
    return CB.rnd("rows.d", tuple(rows.shape)).to(rows.device)


@pytest.mark.parametrize("relu", [False, True])
def test_visual_rows_are_those_of_the_model(dev, relu):
    model, image, taps, _ = build_model(dev, relu)
    seen = []
    model._iqm_branch = lambda xs, vis_cat, *a, **k: seen.append(vis_cat)
    try:
        with torch.no_grad():
            model(image, text_embeddings=torch.zeros(image.shape[0], 256, 2, device=dev))
    finally:
        del model._iqm_branch
    assert len(seen) == 1 and seen[0] is not None                       # the projected form
    rows = autograd.iqm_visual_rows(model, [t.clone().requires_grad_(True) for t in taps])
    B, L, _ = taps[0].shape
    assert rows.shape == (B, len(taps) * (L - 1), model.iqm_hidden_size)
    assert rows.grad_fn is not None and torch.equal(rows.detach(), seen[0])
    if relu:
        assert (rows < 0).any()


@pytest.mark.parametrize("relu", [False, True])
def test_visual_rows_gradients(dev, relu):
    model, image, taps, draw = build_model(dev, relu)
    model.zero_grad(set_to_none=True)
    leaves = [t.clone().requires_grad_(True) for t in taps]
    rows = autograd.iqm_visual_rows(model, leaves)
    d_rows = d_rows_of(rows)
    rows.backward(d_rows)
    ws = [qa.weight for qa in model.query_adapters]
    ln = model.image_encoder.ln_post
    r64, dt64, dw64, zmin = CB.visual_rows_oracle(taps, ws, ln.weight, ln.bias, relu, d_rows, torch.float64)
    _, dt32, dw32, _ = CB.visual_rows_oracle(taps, ws, ln.weight, ln.bias, relu, d_rows, torch.float32)
    e_hip, e_ref = {"rows": rel(rows, r64)}, {}
    for k in range(len(taps)):
        assert not leaves[k].grad[:, 0, :].any()                        # CLS rows: exact zeros
        assert leaves[k].grad[:, 1:, :].any()
        e_hip[f"d_tap.{k}"], e_ref[f"d_tap.{k}"] = rel(leaves[k].grad, dt64[k]), rel(dt32[k], dt64[k])
        e_hip[f"d_weight.{k}"], e_ref[f"d_weight.{k}"] = rel(ws[k].grad, dw64[k]), rel(dw32[k], dw64[k])
    print("iqm_visual_rows relu", relu, "draw", draw, "zmin", zmin, "hip", e_hip, "ref", e_ref)
    PARITY_ERRORS[f"cross_rows_backward.visual_rows.{'leaky' if relu else 'linear'}"] = {"e_hip": e_hip, "e_ref": e_ref}
    for k, e in e_ref.items():
        assert e_hip[k] <= 8 * e, (k, e_hip, e_ref)


def test_fused_and_two_step_routes_are_bit_identical(dev):
    """The LeakyReLU slope applied by aaclip_cross_rows_backward (act set) or by iqm_visual_rows' own backward."""
    model, image, taps, _ = build_model(dev, True)
    B, L, _ = taps[0].shape
    Lk, h, R = len(taps) * (L - 1), model.iqm_hidden_size, 16
    qt = CB.rnd("fused.qt", (B * R, h), 1.5 * h ** -0.5).to(dev)
    d_out = CB.rnd("fused.d_out", (B * R, h)).to(dev)
    grads = []
    for fused in (False, True):
        model.zero_grad(set_to_none=True)
        leaves = [t.clone().requires_grad_(True) for t in taps]
        rows = autograd.iqm_visual_rows(model, leaves, pre_activation_grad=fused)
        out = autograd.cross_rows(qt, rows.view(B * Lk, h), B, R, Lk, act=CB.LEAKY if fused else None)
        out.backward(d_out)
        grads.append([t.grad.clone() for t in leaves] + [qa.weight.grad.clone() for qa in model.query_adapters])
    for a, b in zip(*grads):
        assert a.any() and torch.equal(a, b)


def test_gradient_reaches_the_layer_adapters(dev):
    model, image, _, _ = build_model(dev, False)
    adapters = [m.weight for m in model.image_adapter["layer_adapters"]]
    try:
        for w in adapters:
            w.requires_grad_(True)
        model.zero_grad(set_to_none=True)
        taps = autograd.visual_taps(model, image)
        assert all(t.grad_fn is not None for t in taps)
        rows = autograd.iqm_visual_rows(model, taps)
        rows.backward(d_rows_of(rows))
        for w in adapters:
            assert w.grad is not None and torch.isfinite(w.grad).all() and w.grad.any()
    finally:
        for w in adapters:
            w.requires_grad_(False)
        model.zero_grad(set_to_none=True)
