"""The IQM query-side backward on the GPU: the entry points of csrc/iqm_query_backward.hip against fp64 torch,
autograd.iqm_queries on the reduced model (forward identity, every gradient against fp64 autograd of the oracle's
iqm_branch), train.stage2_loss with the branch's own queries, and train.train_image_adapter.

Bars, the project's own: an entry point against fp64, 1e-4 relative Frobenius on each output (the cases stay within
2.5e-5 in fp32 CPU autograd: tests/test_iqm_query_backward_cpu.py).  Whole-branch gradients with precision fp32: at most
8 x e_ref, e_ref being the oracle's own fp32 CPU autograd against its fp64 autograd, computed in the same test (the rule
of tests/test_gpu_head_backward.py).  Every measured error goes to PARITY_ERRORS under iqm_query_backward.*"""
import functools
import logging

import pytest
import torch

import head_backward_cases as HB
import iqm_query_backward_cases as QB
import oracle.aaclip_oracle as O
import visual_backward_cases as VB
from aaclip_hip import _lib, autograd, engine, synth
from conftest import PARITY_ERRORS
from iqm_query_backward_cases import rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------- the entry points
def run_entry(dev, entry, name, alias=False):
    """-> {output name: tensor or None} of the engine wrapper on the case's inputs"""
    table, _, _, case = QB.ENTRIES[entry]
    c = table[name]
    t = {k: v.to(dev) for k, v in case(name)[0].items()}
    if entry == "small_attention_backward":
        outs = c.get("outs", ("d_q", "d_k", "d_v"))
        d_q, d_k, d_v = engine.small_attention_backward(t["q"], t["k"], t["v"], t["d_out"], c["B"], c["nq"], c["Lk"],
                                                        c["H"], need_q="d_q" in outs, need_k="d_k" in outs,
                                                        need_v="d_v" in outs)
        return {"d_q": d_q, "d_k": d_k, "d_v": d_v}
    if entry == "layernorm_param_grad":
        d_w, d_b = engine.layernorm_param_grad(t["x"], t["d_y"], c["eps"])
        return {"d_w": d_w, "d_b": d_b}
    if entry == "bias_grad":
        return {"db": engine.bias_grad(t["dz"], c["N"])}
    if entry == "act_backward":
        d_y = t["d_y"].clone()
        d_z = engine.act_backward(c["act"], t["zy"], d_y, in_place=alias)
        assert (d_z.data_ptr() == d_y.data_ptr()) == alias
        return {"d_z": d_z}
    d_w, d_b = engine.linear_smallk_backward(t["x"], t["d_y"])
    return {"d_w": d_w, "d_b": d_b}


@pytest.mark.parametrize("entry,name", QB.ALL_CASES)
def test_entry_against_fp64(dev, entry, name):
    want = QB.ENTRIES[entry][3](name)[1]
    got = run_entry(dev, entry, name)
    errs = {}
    for k, w in want.items():
        if w is None:
            assert got[k] is None, k
        elif float(w.norm()) == 0:
            assert not got[k].any(), k                      # one key: ds = 0; a ReLU output of 0: slope 0
            errs[k] = 0.0
        else:
            errs[k] = rel(got[k], w)
    print(entry, name, errs)
    PARITY_ERRORS[f"iqm_query_backward.{entry}.{name}"] = errs
    assert errs and all(v <= 1e-4 for v in errs.values()), errs
    again = run_entry(dev, entry, name)
    for k, v in got.items():
        assert (v is None and again[k] is None) or torch.equal(v, again[k]), k       # two calls: identical bits


def test_exact_zeros(dev):
    got = run_entry(dev, "small_attention_backward", "one_key")
    assert not got["d_q"].any() and not got["d_k"].any() and got["d_v"].any()
    for name, c in QB.ACT.items():
        if c["act"] == QB.RELU:
            z = QB.act_case(name)[0]["zy"].to(dev)
            d_z = run_entry(dev, "act_backward", name)["d_z"]
            assert not d_z[z == 0].any() and torch.equal(d_z[z > 0], QB.act_case(name)[0]["d_y"].to(dev)[z > 0])


def test_single_outputs_equal_the_full_call(dev):
    c = QB.ATTENTION["d_q_only"]
    t = {k: v.to(dev) for k, v in QB.attention_case("d_q_only")[0].items()}
    full = engine.small_attention_backward(t["q"], t["k"], t["v"], t["d_out"], c["B"], c["nq"], c["Lk"], c["H"])
    for i, k in enumerate(("d_q", "d_k", "d_v")):
        one = engine.small_attention_backward(t["q"], t["k"], t["v"], t["d_out"], c["B"], c["nq"], c["Lk"], c["H"],
                                              need_q=i == 0, need_k=i == 1, need_v=i == 2)
        assert [o is not None for o in one] == [j == i for j in range(3)]
        assert torch.equal(one[i], full[i]), k


@pytest.mark.parametrize("name", list(QB.ACT))
def test_aliased_act_backward_equals_the_plain_call(dev, name):
    assert torch.equal(run_entry(dev, "act_backward", name, alias=True)["d_z"], run_entry(dev, "act_backward", name)["d_z"])


def test_bias_grad_ignores_the_padding(dev):
    for name, c in QB.BIAS.items():
        if c["pad"]:
            assert torch.isfinite(run_entry(dev, "bias_grad", name)["db"]).all()


# ---------------------------------------------------------------------------------------------- the whole branch
Z_MARGIN = 2e-6     # tests/test_gpu_cross_rows_backward.py: below this an fp32 pre-activation may sit across the kink
HEADS = 8
UNUSED = ("intermediate.dense", "output.dense", "output.LayerNorm")       # of IQMLayer: the non-query feed-forward


def branch_oracle(taps, anchors, isd, ln_w, ln_b, relu, d_q, dtype):
    """oracle.iqm_branch in `dtype` on the CPU with the taps as leaves, contracted with d_q -> (queries, {name: gradient},
    [d tap], d rows (of the pre-activation rows), smallest |pre-activation| of the LeakyReLU / ReLU inputs).  The rows
    are formed here, with the oracle's own helpers, and handed to iqm_branch as one already projected level (an identity
    query adapter, exact in any dtype), so that their gradient can be read."""
    ts = [t.detach().cpu().to(dtype).requires_grad_(True) for t in taps]
    sd = {k: v.detach().cpu().to(dtype) for k, v in isd.items()}
    leaves = {k: v.requires_grad_(True) for k, v in sd.items() if k not in ("visual_weight", "text_weight")}
    pk = "fc.0" if relu else "fc"
    lw, lb = ln_w.detach().cpu().to(dtype), ln_b.detach().cpu().to(dtype)
    zs, zmin = [], float("inf")
    for k, t in enumerate(ts):
        zs.append(O.layer_norm(t[:, 1:, :], lw, lb) @ leaves[f"query_adapters.{k}.{pk}.weight"].t())
    z = torch.cat(zs, dim=1)
    z.retain_grad()
    if relu:
        zmin = float(z.detach().abs().min())
    rows = O.leaky_relu(z) if relu else z
    z1 = ts[-1][:, 0, :] @ leaves["class_query_mlp.0.weight"].t() + leaves["class_query_mlp.0.bias"]
    zmin = min(zmin, float(z1.detach().abs().min()))
    h = rows.shape[-1]
    inner = {k: v for k, v in leaves.items() if not k.startswith("query_adapters.")}
    inner["query_adapters.0.fc.weight"] = torch.eye(h, dtype=dtype)
    q = O.iqm_branch(ts[-1], [rows], anchors.detach().cpu().to(dtype), inner, relu=False, heads=HEADS, dtype=dtype)
    (q * d_q.detach().cpu().to(dtype)).sum().backward()
    grads = {k: v.grad for k, v in leaves.items()}
    return q.detach(), grads, [t.grad for t in ts], z.grad, zmin


KEY_BIAS_BAR = 1e-12      # the fp64 reference's key.bias gradients against their query.bias siblings: rounding residue


def key_bias_residue(g64):
    """largest |d key.bias| / |d query.bias| over the attentions of the fp64 reference"""
    return max(float(v.norm()) / float(g64[k.replace("key.bias", "query.bias")].norm())
               for k, v in g64.items() if k.endswith("attention.key.bias"))


@functools.lru_cache(maxsize=None)
def build_model(dev, relu, hidden, precision="fp32"):
    """The reduced model of tests/test_gpu_cross_rows_backward.py (image 182, L = 170, D = 256) with the IQM branch
    `hidden` wide and synth_iqm_state_dict loaded: the first seed whose LeakyReLU (query_adapters) and ReLU
    (class_query_mlp) pre-activations all clear Z_MARGIN in fp64 and whose fp64 reference leaves the key.bias gradients
    at half of KEY_BIAS_BAR or less (they are sums that cancel; their residue moves with the summation order of the
    host's fp64 products, so the draw keeps a factor of two) -> (model, image, taps, anchors, isd, draw)"""
    from model.adapter import AdaptedCLIP
    cfg = VB.taps_cfg()
    sd, clip = VB.build_clip(cfg, precision, 7)
    ia = synth.synth_image_adapter_state_dict(cfg, until=VB.TAPS_UNTIL, levels=len(VB.TAPS_LEVELS), relu=relu, seed=7)
    model = AdaptedCLIP(clip, text_adapt_until=1, image_adapt_until=VB.TAPS_UNTIL, levels=VB.TAPS_LEVELS, relu=relu,
                        image_adapt_weight=VB.TAPS_MIX, iqm_hidden_size=hidden, iqm_num_heads=HEADS)
    model.image_adapter.load_state_dict(ia, strict=True)
    for p in model.parameters():
        p.requires_grad_(False)
    model = model.to(dev).eval()
    image, _, anchors, _ = HB.heads_inputs()
    image, anchors = image.to(dev), anchors.float().to(dev)
    taps = [t.detach() for t in autograd.visual_taps(model, image)]
    ln = model.image_encoder.ln_post
    for draw in range(64):
        isd = synth.synth_iqm_state_dict(cfg, levels=len(VB.TAPS_LEVELS), relu=relu, hidden=hidden, seed=111 + draw)
        if precision != "fp32":
            break
        d_q = QB.rnd("branch.d_q", (image.shape[0], 2, hidden))
        _, g64, _, _, zmin = branch_oracle(taps, anchors, isd, ln.weight, ln.bias, relu, d_q, torch.float64)
        if zmin > Z_MARGIN and key_bias_residue(g64) <= 0.5 * KEY_BIAS_BAR:
            break
    else:
        raise AssertionError("no draw clears the kinks")
    missing, unexpected = model.load_state_dict(isd, strict=False)
    assert not unexpected and all(k.startswith(("clipmodel.", "image_encoder.", "image_adapter.", "text_adapter."))
                                  for k in missing)
    return model, image, taps, anchors, isd, draw


def branch_params(model):
    """name (state_dict key relative to the model) -> parameter, for everything the branch owns"""
    return {k: p for k, p in model.named_parameters()
            if k.startswith(("iqm.", "class_query_mlp.", "query_adapters.", "visual_feature_proj.", "text_feature_proj.",
                             "iqm_layer_norm.")) or k in ("pos_embedding", "visual_weight", "text_weight")}


def is_unused(name):
    return name in ("visual_weight", "text_weight") or (
        name.startswith("iqm.encoder.layer.") and name.split(".", 4)[4].startswith(UNUSED))


def d_queries_of(q):
    return QB.rnd("branch.d_q", tuple(q.shape)).to(q.device)


@pytest.mark.parametrize("hidden", [768, 256])
@pytest.mark.parametrize("relu", [False, True])
def test_branch_forward_and_gradients(dev, relu, hidden):
    model, image, taps, anchors, isd, draw = build_model(dev, relu, hidden)
    params = branch_params(model)
    try:
        for p in params.values():
            p.requires_grad_(True)
        model.zero_grad(set_to_none=True)
        with torch.no_grad():
            want_q = model(image, text_embeddings=anchors)[2].last_hidden_state
        leaves = [t.clone().requires_grad_(True) for t in taps]
        q = autograd.iqm_queries(model, leaves, anchors)
        assert q.grad_fn is not None and q.shape == (image.shape[0], 2, hidden) and torch.equal(q.detach(), want_q)
        d_q = d_queries_of(q)
        q.backward(d_q)
        first = {k: (None if p.grad is None else p.grad.clone()) for k, p in params.items()}
        # a second graph with the rows as a leaf: their gradient, and the same bits for every parameter of the query side
        model.zero_grad(set_to_none=True)
        rows = autograd.iqm_visual_rows(model, taps).detach().requires_grad_(True)
        names = autograd._iqm_param_names(model)
        q2 = autograd.IqmQueries.apply(model, rows, taps[-1], anchors, *[params[n] for n in names])
        assert torch.equal(q2.detach(), want_q)
        q2.backward(d_q)
        for n in names:
            assert torch.equal(params[n].grad, first[n]), n
        ln = model.image_encoder.ln_post
        q64, g64, dt64, dr64, zmin = branch_oracle(taps, anchors, isd, ln.weight, ln.bias, relu, d_q, torch.float64)
        _, g32, dt32, dr32, _ = branch_oracle(taps, anchors, isd, ln.weight, ln.bias, relu, d_q, torch.float32)
        assert zmin > Z_MARGIN
        e_hip, e_ref = {"queries": rel(q, q64)}, {}
        qbias = {}
        for k, p in params.items():
            if is_unused(k):
                assert first[k] is None, k
                continue
            assert first[k] is not None and first[k].shape == p.shape and torch.isfinite(first[k]).all(), k
            if k.endswith("crossattention.attention.key.bias"):
                sib = g64[k.replace("key.bias", "query.bias")]
                assert not first[k].any(), k                                   # softmax-invariant: exact zeros
                assert float(g64[k].norm()) <= KEY_BIAS_BAR * float(sib.norm()), k
                continue
            if k.endswith(".attention.attention.key.bias"):
                # the self-attention's key bias is softmax-invariant too: its gradient is the rounding residue of sums
                # that cancel, so it is held against its sibling instead of against itself
                sib = g64[k.replace("key.bias", "query.bias")]
                assert float(g64[k].norm()) <= KEY_BIAS_BAR * float(sib.norm()), k
                qbias[k] = float(first[k].double().norm()) / float(sib.norm())
                assert qbias[k] <= 1e-4, (k, qbias)
                continue
            want = g64[k]
            got = first[k]
            if k == "pos_embedding":
                assert not got[:, 2:].any()
                got, want, ref32 = got[:, :2], want[:, :2], g32[k][:, :2]
            else:
                ref32 = g32[k]
            e_hip[k], e_ref[k] = rel(got, want), rel(ref32, want)
        for i in range(len(taps)):
            e_hip[f"d_tap.{i}"], e_ref[f"d_tap.{i}"] = rel(leaves[i].grad, dt64[i]), rel(dt32[i], dt64[i])
            assert leaves[i].grad[:, 0, :].any() == (i == len(taps) - 1)       # the CLS row: the last tap's alone
        e_hip["d_rows"], e_ref["d_rows"] = rel(rows.grad, dr64), rel(dr32, dr64)
        tag = f"iqm_query_backward.branch.{'leaky' if relu else 'linear'}.h{hidden}"
        print(tag, "draw", draw, "zmin", zmin, "self key.bias", qbias)
        for k in sorted(e_ref):
            print(f"  {k}: hip {e_hip[k]:.3e} ref {e_ref[k]:.3e} ratio {e_hip[k] / max(e_ref[k], 1e-300):.2f}")
        PARITY_ERRORS[tag] = {"e_hip": e_hip, "e_ref": e_ref, "self_key_bias": qbias}
        assert e_hip["queries"] <= 1e-5
        for k, e in e_ref.items():
            assert e_hip[k] <= 8 * e, (k, e_hip[k], e)
    finally:
        for p in params.values():
            p.requires_grad_(False)
        model.zero_grad(set_to_none=True)


@pytest.mark.parametrize("relu", [True, False])
def test_forward_under_fp16x2(dev, relu):
    model, image, taps, anchors, _, _ = build_model(dev, relu, 768, "fp16x2")
    with torch.no_grad():
        want = model(image, text_embeddings=anchors)[2].last_hidden_state
        q = autograd.iqm_queries(model, taps, anchors)
    if relu:
        assert torch.equal(q, want)                       # AdaptedCLIP.forward takes the projected form itself
    else:
        err = (q - want).abs()                            # ... the folded form: tests/test_gpu_iqm.py IQM_HID_TOL
        assert bool((err <= 1.5e-3 + 1e-3 * want.abs()).all()), float(err.max())
        PARITY_ERRORS["iqm_query_backward.fp16x2.folded_vs_projected"] = {"max_abs_err": float(err.max())}


# ---------------------------------------------------------------------------------------------- end to end
def trainable_groups(model):
    """The reference's two optimizer groups (train.py:343-349)"""
    image_params = list(model.image_adapter.parameters())
    iqm_params = (list(model.iqm.parameters()) + list(model.class_query_mlp.parameters())
                  + list(model.query_adapters.parameters()))
    return image_params, iqm_params


def fresh_model(dev):
    model, image, _, anchors, _, _ = build_model.__wrapped__(dev, False, 256)
    for g in trainable_groups(model):
        for p in g:
            p.requires_grad_(True)
    _, mask, _, label = HB.heads_inputs()
    return model, image, mask.float().to(dev), label.to(dev), anchors


def test_stage2_loss_trains_the_branch(dev):
    import train
    model, image, mask, label, anchors = fresh_model(dev)
    loss = train.stage2_loss(model, image, mask, label, anchors, VB.TAPS_IMAGE)
    assert torch.isfinite(loss)
    loss.backward()
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        if is_unused(name):
            assert p.grad is None, name
        elif name.endswith("crossattention.attention.key.bias"):
            assert p.grad is not None and not p.grad.any(), name
        else:
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.any(), name
    with torch.no_grad():
        q = autograd.visual_outputs(model, image, anchors)[2]
    again = train.stage2_loss(model, image, mask, label, anchors, VB.TAPS_IMAGE, q.detach())
    assert torch.equal(again.detach(), loss.detach())


class _Losses(logging.Handler):
    def __init__(self):
        super().__init__()
        self.values = []

    def emit(self, record):
        msg = record.getMessage()
        if msg.startswith("loss: "):
            self.values.append(float(msg[6:]))


def test_train_image_adapter(dev, tmp_path):
    import train
    model, image, mask, label, anchors = fresh_model(dev)
    image_params, iqm_params = trainable_groups(model)
    opt = torch.optim.AdamW([{"params": image_params, "lr": 5e-4},
                             {"params": [p for p in iqm_params], "lr": 5e-5, "weight_decay": 1e-3}], betas=(0.5, 0.999))
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[1], gamma=0.5)
    emb = {"a": anchors[0], "b": anchors[1]}
    batch = {"image": image.cpu(), "mask": mask.cpu(), "label": label.cpu(), "class_name": ["a", "b"]}
    before = {k: v.detach().clone() for k, v in model.state_dict().items() if not k.startswith(("clipmodel.", "image_encoder."))}
    logger = logging.getLogger("test_train_image_adapter")
    logger.setLevel(logging.INFO)
    seen = _Losses()
    logger.addHandler(seen)
    try:
        train.train_image_adapter(model, emb, [batch, batch], opt, sched, str(dev), 0, str(tmp_path), 1, VB.TAPS_IMAGE,
                                  logger)
    finally:
        logger.removeHandler(seen)
    assert len(seen.values) == 1 and seen.values[0] == seen.values[0] and abs(seen.values[0]) < float("inf")
    after = model.state_dict()
    for k in ("image_adapter.seg_proj.0.fc.weight", "image_adapter.layer_adapters.0.fc.0.weight",
              "iqm.encoder.layer.0.attention.attention.query.weight", "class_query_mlp.0.weight",
              "query_adapters.1.fc.weight"):
        assert torch.isfinite(after[k]).all() and not torch.equal(after[k], before[k]), k
    with torch.no_grad():
        trained = model(image, text_embeddings=anchors)[2].last_hidden_state.clone()
    ckpt = torch.load(tmp_path / "image_adapter.pth")
    assert set(ckpt) == {"epoch", "image_adapter", "image_optimizer", "iqm_branch"} and ckpt["epoch"] == 1
    assert (tmp_path / "image_adapter_1.pth").exists()
    model.load_state_dict(before, strict=False)                          # back to the start: other queries
    with torch.no_grad():
        assert not torch.equal(model(image, text_embeddings=anchors)[2].last_hidden_state, trained)
    model.image_adapter.load_state_dict(ckpt["image_adapter"], strict=True)
    train.load_iqm_branch_state(model, ckpt["iqm_branch"])
    with torch.no_grad():
        assert torch.equal(model(image, text_embeddings=anchors)[2].last_hidden_state, trained)


def test_levels_that_stop_short_raise_before_any_launch(dev):
    from model.adapter import AdaptedCLIP
    cfg = VB.taps_cfg()
    _, clip = VB.build_clip(cfg, "fp32", 7)
    model = AdaptedCLIP(clip, text_adapt_until=1, image_adapt_until=VB.TAPS_UNTIL, levels=[1, 2], relu=False).to(dev).eval()
    with pytest.raises(NotImplementedError, match="last block"):
        autograd.iqm_queries(model, [None, None], None)                  # nothing here could be launched on
    with pytest.raises(NotImplementedError, match="last block"):
        autograd.visual_outputs(model, None, None)
