"""CPU side of aaclip_cross_rows_levels_backward: the symbols and the ABI number, the workspace size, the device-free
argument errors (the built library's host code), the conditioning of the cases (fp32 CPU autograd against fp64) and the
kernel's pass sequence in fp64 against autograd."""
import ctypes
import os
import re

import pytest
import torch

import cross_rows_levels_backward_cases as CL
from aaclip_hip import _lib, autograd, engine
from conftest import REPO
from cross_rows_levels_backward_cases import rel

SYMBOLS = ("aaclip_cross_rows_levels_backward_workspace_bytes", "aaclip_cross_rows_levels_backward")
P = 0x7f0000001000      # a plausible, 16-byte aligned device address: nothing here may be dereferenced
BIG = 1 << 40
PREFIX = b"cross_rows_levels_backward:"


def test_symbols_and_abi_version():
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "aaclip.h")).read()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
        assert re.search(r"\b%s\(" % name, header)
    assert callable(engine.cross_rows_levels_backward)
    in_header = int(re.search(r"#define\s+AACLIP_ABI_VERSION\s+(\d+)", header).group(1))
    assert in_header == 10 and lib.aaclip_version() == 10 and _lib.ABI_VERSION == 10


def test_cpu_tensors_raise():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.cross_rows_levels_backward(torch.zeros(4, 768), [torch.zeros(10, 768, dtype=torch.float16)],
                                          torch.zeros(4, 768), 1, 4, 10, 0, 10, 768)


def test_workspace_bytes():
    ws = _lib.load().aaclip_cross_rows_levels_backward_workspace_bytes
    for args in ((0, 16, 4, 100, 768), (2, 0, 4, 100, 768), (2, 16, 0, 100, 768), (2, 16, 4, 0, 768), (2, 16, 4, 100, 0),
                 (-1, 16, 4, 100, 768)):
        assert ws(*args) == 0, args
    base = (2, 8, 3, 1369, 768)
    assert ws(*base) > 0
    grids = ([1, 2, 3, 64, 65535], [4, 8, 12, 16], [1, 2, 3, 4],
             [1, 2, 63, 64, 65, 4096, 8191, 8192, 8193, 8256, 8257, 20000, 100000], [768, 1024])
    for i, values in enumerate(grids):
        sizes = [ws(*(base[:i] + (v,) + base[i + 1:])) for v in values]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (i, sizes)
        assert sizes[0] > 0
    # what the kernels index: SG [B, nseg, Lk, 32], statistics [B, 16, 4] and one partial of d_qt per segment and slice
    for B, R, nseg, Lk, Dk in ((2, 16, 4, 1369, 1024), (2, 12, 2, 64 * CL.MAX_SLICES + 1, 768), (1, 4, 1, 1, 768)):
        per = 64 * -(-Lk // (64 * CL.MAX_SLICES))
        slices = -(-Lk // per)
        assert slices <= CL.MAX_SLICES
        assert ws(B, R, nseg, Lk, Dk) >= 4 * (B * nseg * Lk * 32 + B * 16 * 4 + B * nseg * slices * R * Dk)


def ptr_array(values):
    return (ctypes.c_void_p * len(values))(*values)


def call(lib, x_dtype=1, qt=P, x=(P, P, P, P), nseg=4, d_out=P, d_qt=P, d_x=(P, P, P, P), accumulate=0, B=2, R=16,
         rows_per_image=1370, row0=1, Lk=1369, Dk=1024, ldx=1024, ws=P, ws_bytes=BIG):
    return lib.aaclip_cross_rows_levels_backward(
        x_dtype, qt, None if x is None else ptr_array(x), nseg, d_out, d_qt, None if d_x is None else ptr_array(d_x),
        accumulate, B, R, rows_per_image, row0, Lk, Dk, ldx, ws, ws_bytes, None)


def test_argument_errors():
    """Every check precedes the first launch: these calls carry addresses that are not memory."""
    lib = _lib.load()

    def failed(rc, word):
        msg = lib.aaclip_last_error()
        return rc < 0 and msg.startswith(PREFIX) and word in msg

    for n in ("qt", "x", "d_out", "ws"):
        assert failed(call(lib, **{n: None}), b"null"), n
    assert failed(call(lib, d_qt=None, d_x=None), b"both NULL")
    for n in ("qt", "d_out", "d_qt", "ws"):
        assert failed(call(lib, **{n: P + 4}), b"aligned"), n
    for n in ("x", "d_x"):
        assert failed(call(lib, **{n: (P, P, P + 4, P)}), b"aligned"), n
        assert failed(call(lib, **{n: (P, None, P, P)}), b"non-NULL"), n
    need = lib.aaclip_cross_rows_levels_backward_workspace_bytes(2, 16, 4, 1369, 1024)
    assert failed(call(lib, ws_bytes=need - 1), b"workspace too small")
    assert failed(call(lib, ws_bytes=0), b"workspace too small")
    for kw in (dict(B=0), dict(B=-3), dict(B=65536)):
        assert failed(call(lib, **kw), b"batch"), kw
    for R in (0, 2, 6, 20):
        assert failed(call(lib, R=R), b"effective queries"), R
    for nseg in (0, 5):
        assert failed(call(lib, nseg=nseg), b"segments"), nseg
    assert failed(call(lib, Lk=0), b"no keys")
    for Dk in (256, 512, 640, 2048):
        assert failed(call(lib, Dk=Dk, ldx=2048), b"row width"), Dk
    for ldx in (1023, 1028, 512):
        assert failed(call(lib, ldx=ldx), b"row stride"), ldx
    for dt in (0, 3, -1):
        assert failed(call(lib, x_dtype=dt), b"fp16 or bf16"), dt
    assert failed(call(lib, row0=-1), b"inside an image's rows")
    assert failed(call(lib, row0=2), b"inside an image's rows")
    assert failed(call(lib, rows_per_image=1369), b"inside an image's rows")
    assert failed(call(lib, rows_per_image=1 << 20), b"2 GiB")
    # the accepted edges of the domain fail only for what they lack: a workspace
    for kw in (dict(d_qt=None), dict(d_x=None), dict(ldx=2048), dict(x_dtype=2), dict(R=4), dict(nseg=1), dict(Dk=768, ldx=768)):
        assert failed(call(lib, ws_bytes=0, **kw), b"workspace too small"), kw


@pytest.mark.parametrize("name", list(CL.CASES))
def test_cases_are_well_conditioned(name):
    """fp32 CPU autograd of the reference stays within 2.5e-5 of fp64 on every case: what makes the GPU bar of 1e-4
    attainable on these inputs."""
    c = CL.CASES[name]
    t, want = CL.case(name)
    d_qt, d_x, _ = CL.autograd_reference(name, t, torch.float32)
    got = CL.want_of(name, d_qt, d_x, t)
    errs = {k: rel(got[k], w) for k, w in want.items() if w is not None and float(w.norm()) > 0}
    print(name, errs)
    assert all(v <= 2.5e-5 for v in errs.values()), errs
    if name == "one_key":
        assert not want["d_qt"].any() and not got["d_qt"].any()
    B, R, nseg, Lk, Dk = CL.dims(name)[:5]
    s = CL.scores(t["qt"].double(), [CL.key_rows(v, name).double() for v in t["x"]], B, R, nseg, Dk)
    if c.get("peak") is not None:
        assert float(s.max()) > 79 and float(s.min()) < -40
        assert float(torch.softmax(s, -1).amax(-1).median()) > 0.99          # most rows: one key holds the mass
    elif nseg > 1:
        mass = torch.softmax(s, -1).view(B, R, nseg, Lk).sum(-1)             # every segment takes part in the softmax
        assert float(mass.min()) > 0.01


@pytest.mark.parametrize("name", ["one_key", "two_segments_ragged", "four_segments_bf16", "nearly_one_hot", "offset_rows"])
def test_step_sequence_reproduces_autograd(name):
    t = CL.case_inputs(name)
    d_qt, d_x = CL.step_sequence(name, t)
    r_qt, r_x, _ = CL.autograd_reference(name, t)
    assert rel(torch.stack(d_x), torch.stack(r_x)) <= 1e-12
    assert rel(d_qt, r_qt) <= 1e-12 if float(r_qt.norm()) > 0 else not d_qt.any()


# ---------------------------------------------------------------------------------------------- the folded training route
FOLD_B, FOLD_L, FOLD_D, FOLD_H, FOLD_HEADS, FOLD_LEVELS, FOLD_LT = 2, 6, 768, 256, 4, 2, 11


def folded_stub(width=FOLD_D):
    """The least of an AdaptedCLIP that the folded training route reads (its own _iqm_branch, _iqm_levels and fold rule)
    -> (model, taps [B, L, D] per level, anchors [B, Lt, 2])"""
    from model.adapter import AdaptedCLIP
    from model.adapter_modules import SimpleProj
    from model.iqm import IQM

    class Stub(torch.nn.Module):
        _iqm_branch, _iqm_levels = AdaptedCLIP._iqm_branch, AdaptedCLIP._iqm_levels
        iqm_folds_levels = AdaptedCLIP.iqm_folds_levels

        def __init__(self):
            super().__init__()
            torch.manual_seed(11)
            h = FOLD_H
            self.iqm_hidden_size, self.relu, self.levels, self.code = h, False, [1, 2], _lib.F32
            self.iqm = IQM(hidden_size=h, num_hidden_layers=2, num_attention_heads=FOLD_HEADS, encoder_hidden_size=h,
                           text_encoder_hidden_size=h, intermediate_size=64)
            self.class_query_mlp = torch.nn.Sequential(torch.nn.Linear(width, h), torch.nn.ReLU(), torch.nn.Linear(h, h))
            self.query_adapters = torch.nn.ModuleList([SimpleProj(width, h, False) for _ in range(FOLD_LEVELS)])
            self.visual_feature_proj = torch.nn.Linear(h, h)
            self.text_feature_proj = torch.nn.Linear(2, h)
            self.pos_embedding = torch.nn.Parameter(torch.randn(1, 8, h) * 0.1)
            self.iqm_layer_norm = torch.nn.LayerNorm(h)
            self.image_encoder = torch.nn.Module()
            self.image_encoder.ln_post = torch.nn.LayerNorm(width)
            self.image_encoder.embed_dim = width
            self.image_encoder.transformer = torch.nn.Module()
            self.image_encoder.transformer.resblocks = torch.nn.ModuleList([torch.nn.Identity(), torch.nn.Identity()])
            with torch.no_grad():
                for n, p in self.named_parameters():
                    if n != "pos_embedding":
                        p.normal_(0, (0.6 / p.shape[-1] ** 0.5) if p.dim() > 1 else 0.3)
                for m in self.modules():
                    if isinstance(m, torch.nn.LayerNorm):
                        m.weight.add_(1.0)
            for p in self.image_encoder.parameters():
                p.requires_grad_(False)

        def _code(self):
            return self.code

    g = torch.Generator().manual_seed(12)
    taps = [torch.randn(FOLD_B, FOLD_L, width, generator=g) for _ in range(FOLD_LEVELS)]
    return Stub(), taps, torch.randn(FOLD_B, FOLD_LT, 2, generator=g)


def ln_rows(model, taps):
    ln = model.image_encoder.ln_post
    return [torch.nn.functional.layer_norm(t, (t.shape[-1],), ln.weight, ln.bias, ln.eps).reshape(-1, t.shape[-1]).detach()
            for t in taps]


def test_folded_route_equals_the_oracle_branch(monkeypatch):
    """Every gradient of IqmQueriesFolded, with torch stand-ins for the engine calls (plain fp32, casts the identity),
    against fp64 autograd of the oracle's iqm_branch on the same weights: the algebra of the folded backward, the
    weight-sharing sums for query_adapters (way in and way out, both layers) and visual_feature_proj included."""
    import engine_backward_standins as BS
    from oracle import aaclip_oracle as O
    model, taps, anchors = folded_stub()
    BS.install(monkeypatch)
    names = autograd._iqm_param_names(model)
    params = dict(model.named_parameters())
    leaves = [t.clone().requires_grad_(True) for t in taps]
    qa = [m.weight for m in model.query_adapters]
    out = autograd.IqmQueriesFolded.apply(model, len(taps), anchors, *leaves, *ln_rows(model, taps), *qa,
                                          *[params[n] for n in names])
    d_out = torch.randn(out.shape, generator=torch.Generator().manual_seed(13))
    out.backward(d_out)
    # fp64 autograd of the oracle
    isd = {k: v.detach().double().requires_grad_(v.requires_grad) for k, v in model.state_dict(keep_vars=True).items()}
    t64 = [t.double().requires_grad_(True) for t in taps]
    lw, lb = isd["image_encoder.ln_post.weight"], isd["image_encoder.ln_post.bias"]
    tokens = [O.layer_norm(t[:, 1:, :], lw, lb) for t in t64]
    want = O.iqm_branch(t64[-1], tokens, anchors.double(), isd, relu=False, heads=FOLD_HEADS, dtype=torch.float64)
    (want * d_out.double()).sum().backward()
    errs = {"queries": rel(out, want)}
    for k in range(len(taps)):
        errs[f"d_tap.{k}"] = rel(leaves[k].grad, t64[k].grad)
        errs[f"query_adapters.{k}"] = rel(qa[k].grad, isd[f"query_adapters.{k}.fc.weight"].grad)
        if k < len(taps) - 1:
            assert not leaves[k].grad[:, 0, :].any()                 # CLS rows: exact zeros
    assert leaves[-1].grad[:, 0, :].any()                            # the last tap's: class_query_mlp's share
    for n in names:
        g, w = params[n].grad, isd[n].grad
        if n.endswith("attention.key.bias"):                         # softmax-invariant: zero in exact arithmetic
            assert float(w.norm()) < 1e-12
            if ".attention.attention." in n:                         # the self-attention's comes out of a kernel's sums
                assert float(g.norm()) <= 1e-6 * float(params[n[:-4] + "weight"].grad.norm())
            else:
                assert not g.any()
        elif n == "pos_embedding":
            assert not g[:, 2:].any()
            errs[n] = rel(g[:, :2], w[:, :2])
        else:
            errs[n] = rel(g, w)
    print(errs)
    assert set(names) < set(errs) | {n for n in names if n.endswith("key.bias")}
    assert all(v <= 2.5e-5 for v in errs.values()), {k: v for k, v in errs.items() if v > 2.5e-5}


# the engine calls of one folded visual cross-attention at inference (IQM._attend, enc_levels), in order, at the parent
PARENT_FOLDED_ATTEND = ["gemm", "head_expand", "gemm", "gemm", "gemm", "cross_rows_levels", "gemm", "gemm", "gemm",
                        "head_diag", "gemm", "residual_layernorm"]


def test_record_none_makes_the_parents_calls(monkeypatch):
    """Without a record the folded cross-attention makes the launches it made before it could be recorded, in their
    order, and a record adds none and changes no output."""
    import engine_standins as SI
    model, taps, _ = folded_stub()
    SI.install(monkeypatch)
    levels = model._iqm_levels(ln_rows(model, taps), FOLD_L, _lib.F32)
    vp = model.visual_feature_proj
    h = torch.randn(FOLD_B * 2, FOLD_H, generator=torch.Generator().manual_seed(14))
    att = model.iqm.encoder.layer[0].crossattention
    outs = []
    for record in (None, {}):
        calls = []
        for name in SI.LAUNCHES:
            fn = getattr(SI, name)
            monkeypatch.setattr(engine, name, lambda *a, _n=name, _f=fn, **k: (calls.append(_n), _f(*a, **k))[1])
        with torch.no_grad():
            outs.append(model.iqm._attend(att, h, None, FOLD_B, 2, 0, _lib.F32, enc_proj=(vp.weight, vp.bias),
                                          enc_levels=levels, record=record, key="0.c."))
        assert calls == PARENT_FOLDED_ATTEND, calls
    assert torch.equal(outs[0], outs[1])
    assert set(record) == {"0.c." + k for k in ("qm", "qt", "qx", "u", "tbar", "xbar", "ebar", "ctx", "dense")}
    assert all(t.dtype == torch.float32 for t in record.values())


def test_folded_on_a_model_that_does_not_fold_raises_before_any_call(monkeypatch):
    import engine_backward_standins as BS
    counts = {}
    BS.install(monkeypatch, counts)
    monkeypatch.setattr(engine, "tap_head", lambda *a, **k: counts.__setitem__("tap_head", 1))
    for kind in ("narrow", "fp32", "relu"):
        model, taps, anchors = folded_stub(width=256 if kind == "narrow" else FOLD_D)
        model.code = _lib.F32 if kind == "fp32" else _lib.F16
        model.relu = kind == "relu"
        assert not model.iqm_folds_levels()
        with autograd.use_iqm_train_form("folded"):
            with pytest.raises(NotImplementedError, match="does not fold"):
                autograd.iqm_queries(model, taps, anchors)
            with pytest.raises(NotImplementedError, match="does not fold"):
                autograd.visual_outputs(model, torch.zeros(FOLD_B, 3, 8, 8), anchors)
    assert counts == {}
    model, _, _ = folded_stub()
    model.code = _lib.F16X2
    assert model.iqm_folds_levels()


def test_train_form_selection(monkeypatch):
    assert autograd.iqm_train_form() == "projected"                  # the default: nothing existing changes
    assert autograd.iqm_train_form_from_env({}) == "projected"
    assert autograd.iqm_train_form_from_env({"AACLIP_IQM_TRAIN_FORM": ""}) == "projected"
    assert autograd.iqm_train_form_from_env({"AACLIP_IQM_TRAIN_FORM": "Folded"}) == "folded"
    with pytest.raises(ValueError):
        autograd.iqm_train_form_from_env({"AACLIP_IQM_TRAIN_FORM": "fused"})
    with autograd.use_iqm_train_form("folded"):
        assert autograd.iqm_train_form() == "folded"
        with pytest.raises(ValueError):
            autograd.set_iqm_train_form("other")
        assert autograd.iqm_train_form() == "folded"
    assert autograd.iqm_train_form() == "projected"
    import train
    assert "AACLIP_IQM_TRAIN_FORM" in (train.__doc__ or "") + (train.main.__doc__ or "")
