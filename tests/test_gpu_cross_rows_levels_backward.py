"""aaclip_cross_rows_levels_backward on the GPU against fp64 torch autograd of the forward formula on the exact 16-bit
row values (tests/cross_rows_levels_backward_cases.py), and the folded training route of the IQM branch
(autograd.iqm_train_form "folded") on a reduced model whose forward folds: forward identity with AdaptedCLIP.forward,
every gradient against the fp64 oracle, stage2_loss, one train_image_adapter epoch, and the folded forward at D = 768.

Bar, the project's own for every backward entry: 1e-4 relative Frobenius on each output (the cases stay within 2.5e-5
in fp32 CPU autograd: tests/test_cross_rows_levels_backward_cpu.py).  Every measured error goes to PARITY_ERRORS under
cross_rows_levels_backward.*"""
import functools
import logging

import pytest
import torch
import torch.nn.functional as F

import cross_rows_levels_backward_cases as CL
from aaclip_hip import autograd, engine, synth
from conftest import PARITY_ERRORS
from cross_rows_levels_backward_cases import rel
from oracle import aaclip_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def level_buffers(x, name):
    """the case's rows as engine.cross_rows_levels takes them: 16-bit rows, or uint8 split8 rows for a stride of 2 Dk"""
    Dk, ldx = CL.dims(name)[4], CL.dims(name)[7]
    return [v.view(torch.uint8) for v in x] if ldx == 2 * Dk else x


def run_case(dev, name, base=True):
    """-> {d_qt, d_x: the list of whole level buffers} of engine.cross_rows_levels_backward on the case's inputs.  Every
    buffer starts as SENTINEL; an accumulate case then takes its base in the key rows and the call adds, every other
    case (and base=False) has the call overwrite the key rows."""
    c = CL.CASES[name]
    B, R, nseg, Lk, Dk, rpi, row0, ldx, code = CL.dims(name)
    t = CL.case(name)[0]
    x = level_buffers([v.to(dev) for v in t["x"]], name)
    outs = c.get("outs", "both")
    d_x = None
    if outs != "d_qt":
        d_x = [torch.full((B * rpi, Dk), CL.SENTINEL, dtype=torch.float32, device=dev) for _ in range(nseg)]
        if c.get("accumulate") and base:
            for s, g in enumerate(d_x):
                CL.key_rows(g, name).copy_(CL.key_rows(t["base"][s], name))
    d_qt, d_x = engine.cross_rows_levels_backward(t["qt"].to(dev), x, t["d_out"].to(dev), B, R, rpi, row0, Lk, Dk,
                                                  need_qt=outs != "d_x", need_x=outs != "d_qt", d_x=d_x,
                                                  overwrite=not (c.get("accumulate") and base))
    return {"d_qt": d_qt, "d_x": d_x}


def key_part(d_x, name):
    return torch.stack([CL.key_rows(g, name) for g in d_x])


@pytest.mark.parametrize("name", list(CL.CASES))
def test_against_fp64(dev, name):
    want = CL.case(name)[1]
    got = run_case(dev, name)
    got_k = {"d_qt": got["d_qt"], "d_x": None if got["d_x"] is None else key_part(got["d_x"], name)}
    errs = {}
    for k, w in want.items():
        if w is None:
            assert got_k[k] is None, k
        elif float(w.norm()) == 0:
            assert not got_k[k].any(), k                    # one key: ds = 0 and d_qt = 0 exactly
            errs[k] = 0.0
        else:
            errs[k] = rel(got_k[k], w)
    print("cross_rows_levels_backward", name, errs)
    PARITY_ERRORS[f"cross_rows_levels_backward.{name}"] = errs
    assert errs and all(v <= 1e-4 for v in errs.values()), errs


@pytest.mark.parametrize("name", ["production", "two_segments_ragged", "four_segments_bf16", "split8_r12"])
def test_two_calls_are_bit_identical(dev, name):
    a, b = run_case(dev, name), run_case(dev, name)
    assert torch.equal(a["d_qt"], b["d_qt"])
    for ga, gb in zip(a["d_x"], b["d_x"]):
        assert torch.equal(ga, gb)


def test_accumulate_adds_onto_the_buffer(dev):
    name = "accumulate"
    base = torch.stack([CL.key_rows(b, name) for b in CL.case(name)[0]["base"]]).to(dev)
    acc, plain = run_case(dev, name), run_case(dev, name, base=False)
    assert torch.equal(acc["d_qt"], plain["d_qt"])
    a, p = key_part(acc["d_x"], name), key_part(plain["d_x"], name)
    want = base.double() + p.double()                               # exact in fp64: the one rounding is the kernel's
    ulp = torch.finfo(torch.float32).eps * want.abs().clamp_min(torch.finfo(torch.float32).tiny)
    assert ((a.double() - want).abs() <= ulp).all()
    assert not torch.equal(a, p)


@pytest.mark.parametrize("name", ["offset_rows", "accumulate", "production"])
def test_rows_outside_the_key_range_keep_their_sentinel(dev, name):
    B, _, _, Lk, Dk, rpi, row0, _, _ = CL.dims(name)
    assert rpi > Lk
    for g in run_case(dev, name)["d_x"]:
        g = g.view(B, rpi, Dk)
        assert (g[:, :row0] == CL.SENTINEL).all() and (g[:, row0 + Lk:] == CL.SENTINEL).all()
        assert (g[:, row0:row0 + Lk] != CL.SENTINEL).all()


def test_one_key_d_qt_is_exactly_zero(dev):
    got = run_case(dev, "one_key")
    assert not got["d_qt"].any()
    assert key_part(got["d_x"], "one_key").any()


def test_buffers_made_by_the_engine_are_zero_outside_the_keys(dev):
    name = "offset_rows"
    B, R, nseg, Lk, Dk, rpi, row0, _, _ = CL.dims(name)
    t = CL.case(name)[0]
    _, d_x = engine.cross_rows_levels_backward(t["qt"].to(dev), [v.to(dev) for v in t["x"]], t["d_out"].to(dev), B, R,
                                               rpi, row0, Lk, Dk, need_qt=False)
    ref = run_case(dev, name)["d_x"]
    for g, r in zip(d_x, ref):
        assert not g.view(B, rpi, Dk)[:, :row0].any()
        assert torch.equal(CL.key_rows(g, name), CL.key_rows(r, name))


# ---------------------------------------------------------------------------------------------- the folded training route
# A reduced model whose forward folds: a vision tower 768 wide (2 blocks, 12 heads), image 70 (grid 5, L = 26), taps
# after both blocks, one layer adapter, 8 IQM heads (R = 16).
HEADS, LEVELS, UNTIL, MIX, IMAGE, BATCH = 8, (1, 2), 1, 0.1, 70, 2
UNUSED = ("intermediate.dense", "output.dense", "output.LayerNorm")       # of IQMLayer: the non-query feed-forward


def fold_cfg():
    return synth.ClipCfg(embed_dim=256, image_size=IMAGE, vision=synth.TowerCfg(768, 2, 12, 3072),
                         text=synth.TowerCfg(256, 1, 4, 1024))


@functools.lru_cache(maxsize=None)
def build_model(dev, precision, hidden):
    """-> (model with nothing trainable, image, anchors [B, E, 2], CLIP state dict, image adapter state dict, IQM one)"""
    from model.adapter import AdaptedCLIP
    from model.model import CLIP
    cfg = fold_cfg()
    sd = synth.synth_clip_state_dict(cfg, seed=7)
    clip = CLIP(cfg.embed_dim, dict(image_size=cfg.image_size, layers=cfg.vision.layers, width=cfg.vision.width,
                                    patch_size=cfg.patch_size),
                dict(context_length=77, vocab_size=cfg.vocab_size, width=cfg.text.width, heads=cfg.text.heads,
                     layers=cfg.text.layers), precision=precision)
    clip.load_state_dict(sd, strict=True)
    ia = synth.synth_image_adapter_state_dict(cfg, until=UNTIL, levels=len(LEVELS), relu=False, seed=7)
    isd = synth.synth_iqm_state_dict(cfg, levels=len(LEVELS), relu=False, hidden=hidden, seed=113)
    model = AdaptedCLIP(clip, text_adapt_until=1, image_adapt_until=UNTIL, levels=list(LEVELS), relu=False,
                        image_adapt_weight=MIX, iqm_hidden_size=hidden, iqm_num_heads=HEADS)
    model.image_adapter.load_state_dict(ia, strict=True)
    missing, unexpected = model.load_state_dict(isd, strict=False)
    assert not unexpected and all(k.startswith(("clipmodel.", "image_encoder.", "image_adapter.", "text_adapter."))
                                  for k in missing)
    for p in model.parameters():
        p.requires_grad_(False)
    model = model.to(dev).eval()
    image = synth.synth_images(BATCH, IMAGE, seed=7).to(dev)
    t = CL.rnd("fold.anchors", (BATCH, cfg.embed_dim, 2)).double()
    anchors = (t / t.norm(dim=1, keepdim=True)).float().to(dev)
    return model, image, anchors, sd, ia, isd


def branch_params(model):
    return {k: p for k, p in model.named_parameters()
            if k.startswith(("iqm.", "class_query_mlp.", "query_adapters.", "visual_feature_proj.", "text_feature_proj.",
                             "iqm_layer_norm.")) or k == "pos_embedding"}


def is_unused(name):
    return name in ("visual_weight", "text_weight") or (
        name.startswith("iqm.encoder.layer.") and name.split(".", 4)[4].startswith(UNUSED))


@pytest.mark.parametrize("hidden", [256, 768])
@pytest.mark.parametrize("precision", ["fp16", "bf16", "fp16x2"])
def test_folded_training_queries_are_the_forwards_bits(dev, precision, hidden):
    model, image, anchors, _, _, _ = build_model(dev, precision, hidden)
    assert model.iqm_folds_levels()
    with torch.no_grad():
        want = model(image, text_embeddings=anchors)[2].last_hidden_state
    taps = autograd.visual_taps(model, image)
    assert autograd.iqm_train_form() == "projected"
    q_proj = autograd.iqm_queries(model, taps, anchors)
    rows = autograd.iqm_visual_rows(model, taps, pre_activation_grad=False)
    params = dict(model.named_parameters())
    direct = autograd.IqmQueries.apply(model, rows, taps[-1], anchors,
                                       *[params[n] for n in autograd._iqm_param_names(model)])
    assert torch.equal(q_proj, direct)                       # the projected route's queries stay what they are
    with autograd.use_iqm_train_form("folded"):
        q = autograd.iqm_queries(model, taps, anchors)
        seg, det, q2 = autograd.visual_outputs(model, image, anchors)
    assert q.shape == (BATCH, 2, hidden) and torch.equal(q, want) and torch.equal(q2, want)
    with torch.no_grad():
        seg0, det0, _ = model(image)
    assert torch.equal(det, det0) and all(torch.equal(a, b) for a, b in zip(seg, seg0))
    assert not torch.equal(q_proj, want)                     # two forwards: what the folded form is for


# ---- gradients: the HIP route and a CPU emulation of the forward's 16-bit roundings, both against the fp64 oracle
def oracle_branch(taps, anchors, isd, ln_w, ln_b, d_q):
    """oracle.iqm_branch in fp64 on the CPU with the taps as leaves -> (queries, {name: gradient}, [d tap])"""
    ts = [t.detach().cpu().double().requires_grad_(True) for t in taps]
    leaves = {k: v.detach().cpu().double().requires_grad_(True) for k, v in isd.items()
              if k not in ("visual_weight", "text_weight")}
    lw, lb = ln_w.detach().cpu().double(), ln_b.detach().cpu().double()
    tokens = [O.layer_norm(t[:, 1:, :], lw, lb) for t in ts]
    q = O.iqm_branch(ts[-1], tokens, anchors.detach().cpu().double(), leaves, relu=False, heads=HEADS, dtype=torch.float64)
    (q * d_q.detach().cpu().double()).sum().backward()
    return q.detach(), {k: v.grad for k, v in leaves.items()}, [t.grad for t in ts]


def emulated_branch(taps, anchors, isd, ln_w, ln_b, d_q, precision):
    """The folded forward of AdaptedCLIP._iqm_branch / IQM._attend written in fp32 torch on the CPU, rounding to 16 bits
    where the forward does (straight-through: the value is rounded, the gradient passes): the LayerNorm'ed tap rows and
    the probabilities of the visual cross-attention under every precision; under fp16 / bf16 also both operands of every
    product of the branch (under fp16x2 the branch's products are fp32).  -> ({name: gradient}, [d tap])"""
    dt16 = torch.bfloat16 if precision == "bf16" else torch.float16

    def st(x, dt):
        return x + (x.detach().to(dt).to(x.dtype) - x.detach())

    r_row = lambda x: st(x, dt16)
    r = (lambda x: x) if precision == "fp16x2" else (lambda x: st(x, dt16))
    ts = [t.detach().cpu().float().requires_grad_(True) for t in taps]
    sd = {k: v.detach().cpu().float().requires_grad_(True) for k, v in isd.items() if k not in ("visual_weight", "text_weight")}
    lw, lb = ln_w.detach().cpu().float(), ln_b.detach().cpu().float()
    B, h = ts[0].shape[0], sd["iqm_layer_norm.weight"].shape[0]
    hd = h // HEADS

    def lin(x, name, bias=True):
        y = r(x) @ r(sd[name + ".weight"]).t()
        return y + sd[name + ".bias"] if bias else y

    def ln(x, name, eps):
        return F.layer_norm(x, (x.shape[-1],), sd[name + ".weight"], sd[name + ".bias"], eps)

    def expand(q):                                           # head_expand: [B, nq, h] -> [B, nq * H, h]
        m = torch.zeros(HEADS, h)
        for i in range(HEADS):
            m[i, i * hd:(i + 1) * hd] = hd ** -0.5
        return (q.unsqueeze(2) * m).reshape(B, -1, h)

    def diag(full):                                          # head_diag: [B, nq * H, h] -> [B, nq, h]
        f = full.view(B, -1, HEADS, h)
        return torch.cat([f[:, :, i, i * hd:(i + 1) * hd] for i in range(HEADS)], -1)

    def tail(p, hin, ebar):
        ctx = diag(lin(ebar, p + "attention.value"))
        return ln(lin(ctx, p + "output.dense") + hin, p + "output.LayerNorm", 1e-12)

    def self_attention(p, hin):                              # k and v are stored in the compute dtype, q stays fp32
        q, k, v = (lin(hin, p + "attention." + n).view(B, -1, HEADS, hd).transpose(1, 2) for n in ("query", "key", "value"))
        a = torch.softmax(q @ r(k).transpose(-1, -2) / hd ** 0.5, -1)
        ctx = (a @ r(v)).transpose(1, 2).reshape(B, -1, h)
        return ln(lin(ctx, p + "output.dense") + hin, p + "output.LayerNorm", 1e-12)

    rows = [r_row(F.layer_norm(t[:, 1:, :], (t.shape[-1],), lw, lb, 1e-5)) for t in ts]
    wqa = [sd[f"query_adapters.{k}.fc.weight"] for k in range(len(ts))]
    vp_w, vp_b = sd["visual_feature_proj.weight"], sd["visual_feature_proj.bias"]

    def visual(p, hin):
        qt = r(expand(lin(hin, p + "attention.query"))) @ r(sd[p + "attention.key.weight"])
        qx = r(qt) @ r(vp_w)
        s = torch.cat([(r(qx) @ r(w)) @ x.transpose(1, 2) for w, x in zip(wqa, rows)], -1)
        e = torch.exp(s - s.amax(-1, keepdim=True).detach())
        n = rows[0].shape[1]
        tbar = [(st(e[..., k * n:(k + 1) * n], dt16) @ x) / e.sum(-1, keepdim=True) for k, x in enumerate(rows)]
        xbar = sum(r(t) @ r(w).t() for t, w in zip(tbar, wqa))
        return tail(p, hin, r(xbar) @ r(vp_w).t() + vp_b)

    txt = r(anchors.detach().cpu().float() @ sd["text_feature_proj.weight"].t() + sd["text_feature_proj.bias"])

    def text(p, hin):
        qt = r(expand(lin(hin, p + "attention.query"))) @ r(sd[p + "attention.key.weight"])
        a = torch.softmax(qt @ txt.transpose(1, 2), -1)
        return tail(p, hin, a @ txt)

    cq = lin(torch.relu(lin(ts[-1][:, 0, :], "class_query_mlp.0")), "class_query_mlp.2")
    hcur = ln(cq.unsqueeze(1) + sd["pos_embedding"][:, :2, :], "iqm.layernorm", 1e-12)
    for l in range(2):
        p = f"iqm.encoder.layer.{l}."
        a = self_attention(p + "attention.", hcur)
        c = visual(p + "crossattention.", a)
        t = text(p + "text_crossattention.", c)
        mix = 0.4 * a + 0.3 * c + 0.3 * t
        inter = O.gelu_erf(lin(mix, p + "intermediate_query.dense"))
        hcur = ln(lin(inter, p + "output_query.dense") + mix, p + "output_query.LayerNorm", 1e-12)
    q = ln(hcur, "iqm_layer_norm", 1e-5)
    (q * d_q.detach().cpu().float()).sum().backward()
    return q.detach(), {k: v.grad for k, v in sd.items()}, [t.grad for t in ts]


@pytest.mark.parametrize("precision,hidden", [("fp16x2", 256), ("fp16x2", 768), ("fp16", 256), ("bf16", 256)])
def test_folded_gradients_against_the_fp64_oracle(dev, precision, hidden):
    """Bar per gradient: 4 x the error of the CPU emulation above against the same fp64 oracle, measured here.  The
    margin covers summation order and the kernel's unnormalised fp16 probabilities."""
    model, image, anchors, _, _, isd = build_model(dev, precision, hidden)
    params = branch_params(model)
    try:
        for p in params.values():
            p.requires_grad_(True)
        model.zero_grad(set_to_none=True)
        taps = [t.detach() for t in autograd.visual_taps(model, image)]
        leaves = [t.clone().requires_grad_(True) for t in taps]
        with autograd.use_iqm_train_form("folded"):
            q = autograd.iqm_queries(model, leaves, anchors)
        d_q = CL.rnd("fold.d_q", tuple(q.shape)).to(dev)
        q.backward(d_q)
        lnp = model.image_encoder.ln_post
        q64, g64, dt64 = oracle_branch(taps, anchors, isd, lnp.weight, lnp.bias, d_q)
        qe, ge, dte = emulated_branch(taps, anchors, isd, lnp.weight, lnp.bias, d_q, precision)
        e_hip, e_emu = {"queries": rel(q, q64)}, {"queries": rel(qe, q64)}
        for k, p in params.items():
            if is_unused(k):
                assert p.grad is None, k
                continue
            assert p.grad is not None and torch.isfinite(p.grad).all(), k
            if k.endswith("attention.key.bias"):             # softmax-invariant: exact zeros / rounding residue
                if "crossattention" in k:
                    assert not p.grad.any(), k
                continue
            got, want, emu = p.grad, g64[k], ge[k]
            if k == "pos_embedding":
                assert not got[:, 2:].any()
                got, want, emu = got[:, :2], want[:, :2], emu[:, :2]
            e_hip[k], e_emu[k] = rel(got, want), rel(emu, want)
        for i in range(len(taps)):
            e_hip[f"d_tap.{i}"], e_emu[f"d_tap.{i}"] = rel(leaves[i].grad, dt64[i]), rel(dte[i], dt64[i])
            assert leaves[i].grad[:, 0, :].any() == (i == len(taps) - 1)       # the CLS rows: the last tap's alone
        tag = f"cross_rows_levels_backward.folded_gradients.{precision}.h{hidden}"
        print(tag)
        for k in sorted(e_emu):
            print(f"  {k}: hip {e_hip[k]:.3e} emulation {e_emu[k]:.3e} ratio {e_hip[k] / max(e_emu[k], 1e-300):.2f}")
        PARITY_ERRORS[tag] = {"e_hip": e_hip, "e_emulation": e_emu}
        for k, e in e_emu.items():
            assert e_hip[k] <= 4 * e, (k, e_hip[k], e)
    finally:
        for p in params.values():
            p.requires_grad_(False)
        model.zero_grad(set_to_none=True)


# ---- end to end
def trainable_groups(model):
    """The reference's two optimizer groups (train.py:343-349)"""
    image_params = list(model.image_adapter.parameters())
    iqm_params = (list(model.iqm.parameters()) + list(model.class_query_mlp.parameters())
                  + list(model.query_adapters.parameters()))
    return image_params, iqm_params


def fresh_model(dev, precision="fp16x2"):
    model, image, anchors, _, _, _ = build_model.__wrapped__(dev, precision, 256)
    for g in trainable_groups(model):
        for p in g:
            p.requires_grad_(True)
    S = IMAGE
    mask = torch.zeros(BATCH, 1, S, S)
    for b in range(BATCH):
        mask[b, 0, 10 + 9 * b:10 + 9 * b + S // 3, 8 + 5 * b:8 + 5 * b + S // 2] = 1
    return model, image, mask.to(dev), torch.tensor([1, 0]).to(dev), anchors


def test_stage2_loss_under_the_folded_form(dev):
    import train
    model, image, mask, label, anchors = fresh_model(dev)
    grads = []
    with autograd.use_iqm_train_form("folded"):
        for _ in range(2):
            model.zero_grad(set_to_none=True)
            loss = train.stage2_loss(model, image, mask, label, anchors, IMAGE)
            assert torch.isfinite(loss)
            loss.backward()
            grads.append({k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        if is_unused(name):
            assert p.grad is None, name
        elif name.endswith("crossattention.attention.key.bias"):
            assert p.grad is not None and not p.grad.any(), name
        else:
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.any(), name
    assert grads[0].keys() == grads[1].keys()
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k       # a second backward: the same bits
    with torch.no_grad():
        q = model(image, text_embeddings=anchors)[2].last_hidden_state
        again = train.stage2_loss(model, image, mask, label, anchors, IMAGE, q)
    assert torch.equal(again, loss.detach())                  # the loss saw the forward's own queries


def test_train_image_adapter_under_the_folded_form(dev, tmp_path):
    import train
    model, image, mask, label, anchors = fresh_model(dev)
    image_params, iqm_params = trainable_groups(model)
    opt = torch.optim.AdamW([{"params": image_params, "lr": 5e-4},
                             {"params": iqm_params, "lr": 5e-5, "weight_decay": 1e-3}], betas=(0.5, 0.999))
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[1], gamma=0.5)
    emb = {"a": anchors[0], "b": anchors[1]}
    batch = {"image": image.cpu(), "mask": mask.cpu(), "label": label.cpu(), "class_name": ["a", "b"]}
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    logger = logging.getLogger("test_train_image_adapter_folded")
    with autograd.use_iqm_train_form("folded"):
        train.train_image_adapter(model, emb, [batch, batch], opt, sched, str(dev), 0, str(tmp_path), 1, IMAGE, logger)
    after = model.state_dict()
    for k in ("image_adapter.seg_proj.0.fc.weight", "image_adapter.layer_adapters.0.fc.0.weight",       # group 1
              "iqm.encoder.layer.0.crossattention.attention.key.weight", "class_query_mlp.0.weight",     # group 2
              "query_adapters.0.fc.weight", "query_adapters.1.fc.weight"):
        assert torch.isfinite(after[k]).all() and not torch.equal(after[k], before[k]), k


# ---- inference only: the folded forward at D = 768 against the fp64 oracle (DESIGN.md section 10's open note)
IQM_HID_TOL = {"fp16x2": (1.5e-3, 1e-3), "fp16": (2e-2, 2e-2)}      # tests/test_gpu_iqm.py


@pytest.mark.parametrize("precision", ["fp16x2", "fp16"])
def test_folded_forward_at_768_against_the_fp64_oracle(dev, precision):
    model, image, anchors, sd, ia, isd = build_model(dev, precision, 768)
    assert model.iqm_folds_levels()
    with torch.no_grad():
        h = model(image, text_embeddings=anchors)[2].last_hidden_state
    seg, det, stream = O.adapted_visual_forward(image.cpu(), sd, ia, 12, MIX, UNTIL, LEVELS, relu=False,
                                                dtype=torch.float64, return_stream=True)
    lw, lb = sd["visual.ln_post.weight"].double(), sd["visual.ln_post.bias"].double()
    tokens = [O.layer_norm(x[:, 1:, :], lw, lb) for x in stream]
    ref = O.iqm_branch(stream[-1], tokens, anchors.cpu().double(), isd, relu=False, heads=HEADS, dtype=torch.float64)
    err = (h.double().cpu() - ref).abs()
    atol, rtol = IQM_HID_TOL[precision]
    PARITY_ERRORS[f"cross_rows_levels_backward.folded_forward_768.{precision}"] = {
        "max_abs_err": float(err.max()), "rms_err": float(err.pow(2).mean().sqrt()), "ref_std": float(ref.std())}
    print("folded forward at 768", precision, "max |err|", float(err.max()), "ref std", float(ref.std()))
    bad = err > atol + rtol * ref.abs()
    assert not bad.any(), f"{int(bad.sum())}/{bad.numel()} outside {atol}+{rtol}|ref|, max err {float(err.max()):.3e}"
