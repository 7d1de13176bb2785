"""CPU side of the IQM query-side backward: the new symbols and their signatures, the Python surface, the workspace
sizes, every device-free argument error of every new entry, the conditioning of the cases (fp32 CPU autograd against
fp64), stage2_loss with given queries, train_image_adapter's call order and checkpoint with a stub model and loss, and
the one forward of the query side with and without a record (outputs, keys and the calls per engine function)."""
import ctypes as C
import inspect
import logging
import os
import re

import pytest
import torch

import iqm_query_backward_cases as QB
from aaclip_hip import _lib, autograd, engine
from conftest import REPO
from iqm_query_backward_cases import rel

SYMBOLS = {
    "aaclip_small_attention_backward": 14,
    "aaclip_layernorm_param_grad_workspace_bytes": 2,
    "aaclip_layernorm_param_grad": 10,
    "aaclip_bias_grad_workspace_bytes": 2,
    "aaclip_bias_grad": 8,
    "aaclip_act_backward": 6,
    "aaclip_linear_smallk_backward_workspace_bytes": 3,
    "aaclip_linear_smallk_backward": 10,
}
SURFACE = ((engine, "small_attention_backward"), (engine, "layernorm_param_grad"), (engine, "bias_grad"),
           (engine, "act_backward"), (engine, "linear_smallk_backward"), (autograd, "IqmQueries"),
           (autograd, "iqm_queries"), (autograd, "visual_outputs"))
P = 0x7f0000001000      # a plausible, 16-byte aligned device address: nothing here may be dereferenced
BIG = 1 << 40


def test_symbols_signatures_and_abi_version():
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "aaclip.h")).read()
    for name, nargs in SYMBOLS.items():
        res, args = _lib.SIGNATURES[name]
        assert len(args) == nargs, name
        assert res is (C.c_size_t if name.endswith("_workspace_bytes") else C.c_int), name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
        decl = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert decl and decl.group(1).count(",") + 1 == nargs, name
    for mod, name in SURFACE:
        assert callable(getattr(mod, name))
    in_header = int(re.search(r"#define\s+AACLIP_ABI_VERSION\s+(\d+)", header).group(1))
    assert in_header == 10 and lib.aaclip_version() == 10 and _lib.ABI_VERSION == 10
    assert _lib.ACT_GELU == QB.GELU == 3 and _lib.ACT_RELU == QB.RELU
    assert engine.SMALL_ATTENTION_BACKWARD_MAX_KEYS == QB.MAX_KEYS
    assert "taps" in inspect.signature(autograd.visual_heads).parameters


def test_cpu_tensors_raise():
    z = torch.zeros
    for call in (lambda: engine.small_attention_backward(z(2, 32), z(2, 32), z(2, 32), z(2, 32), 1, 2, 2, 1),
                 lambda: engine.layernorm_param_grad(z(4, 256), z(4, 256), 1e-5),
                 lambda: engine.bias_grad(z(4, 256)),
                 lambda: engine.act_backward(_lib.ACT_GELU, z(8), z(8)),
                 lambda: engine.linear_smallk_backward(z(4, 2), z(4, 64))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_workspace_bytes():
    lib = _lib.load()
    ln, bias, sk = (lib.aaclip_layernorm_param_grad_workspace_bytes, lib.aaclip_bias_grad_workspace_bytes,
                    lib.aaclip_linear_smallk_backward_workspace_bytes)
    for fn, empties in ((ln, ((0, 768), (4, 0), (-1, 768), (4, -64))), (bias, ((0, 768), (4, 0), (-2, 768))),
                        (sk, ((0, 768, 2), (4, 0, 2), (4, 768, 0), (-1, 768, 2)))):
        for args in empties:
            assert fn(*args) == 0, args
    rows = [1, 2, 31, 32, 33, 64, 130, 2047, 2048, 2049, 4096, 100000, 1 << 24]
    for fn, base, grids in ((ln, (4, 768), (rows, [64, 256, 768, 1024, 4096])),
                            (bias, (4, 768), (rows, [1, 64, 768, 2048, 5000])),
                            (sk, (1536, 768, 2), (rows, [1, 64, 768, 2048], [1, 2, 3, 4]))):
        assert fn(*base) > 0
        for i, values in enumerate(grids):
            sizes = [fn(*(base[:i] + (v,) + base[i + 1:])) for v in values]
            assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), (fn, i, sizes)
    # what the kernels index: one partial row per chunk (and the per-row statistics of the LayerNorm)
    for r in (1, 4, 130, 2 * 768 + 3, 5000):
        ch = QB.chunks_of(r)
        assert 1 <= ch <= QB.MAX_CHUNKS and ch * -(-r // ch) >= r
        assert ln(r, 768) >= 4 * (2 * r + ch * 2 * 768)
        assert bias(r, 2048) >= 4 * ch * 2048
        assert sk(r, 768, 2) >= 4 * ch * 768 * 3


def failed(lib, rc, prefix, word):
    msg = lib.aaclip_last_error()
    return rc < 0 and msg.startswith(prefix) and word in msg


def test_small_attention_backward_argument_errors():
    """Every check precedes the first launch: these calls carry addresses that are not memory."""
    lib = _lib.load()
    pre = b"small_attention_backward:"

    def call(q=P, k=P, v=P, d_out=P, d_q=P, d_k=P, d_v=P, B=2, nq=2, Lk=2, H=8, hd=96, scale=0.1):
        return lib.aaclip_small_attention_backward(q, k, v, d_out, d_q, d_k, d_v, B, nq, Lk, H, hd, scale, None)

    for n in ("q", "k", "v", "d_out"):
        assert failed(lib, call(**{n: None}), pre, b"null"), n
    assert failed(lib, call(d_q=None, d_k=None, d_v=None), pre, b"all NULL")
    for n in ("q", "k", "v", "d_out", "d_q", "d_k", "d_v"):
        assert failed(lib, call(**{n: P + 4}), pre, b"aligned"), n
    for kw in (dict(B=0), dict(nq=0), dict(Lk=0), dict(H=0), dict(hd=0), dict(B=-1)):
        assert failed(lib, call(**kw), pre, b"empty"), kw
    assert failed(lib, call(B=65536), pre, b"grid limit") and failed(lib, call(H=65536), pre, b"grid limit")
    assert failed(lib, call(nq=5), pre, b"queries")
    assert failed(lib, call(Lk=257), pre, b"keys")
    for hd in (2, 6, 132, 256):
        assert failed(lib, call(hd=hd), pre, b"head size"), hd


def test_layernorm_param_grad_argument_errors():
    lib = _lib.load()
    pre = b"layernorm_param_grad:"

    def call(x=P, d_y=P, d_w=P, d_b=P, rows=4, D=768, eps=1e-5, ws=P, ws_bytes=BIG):
        return lib.aaclip_layernorm_param_grad(x, d_y, d_w, d_b, rows, D, eps, ws, ws_bytes, None)

    for n in ("x", "d_y", "ws"):
        assert failed(lib, call(**{n: None}), pre, b"null"), n
    assert failed(lib, call(d_w=None, d_b=None), pre, b"both NULL")
    for n in ("x", "d_y", "d_w", "d_b", "ws"):
        assert failed(lib, call(**{n: P + 8}), pre, b"aligned"), n
    for kw in (dict(rows=0), dict(D=0), dict(rows=-4)):
        assert failed(lib, call(**kw), pre, b"empty"), kw
    for D in (32, 100, 4160):
        assert failed(lib, call(D=D), pre, b"multiple of 64"), D
    need = lib.aaclip_layernorm_param_grad_workspace_bytes(4, 768)
    assert failed(lib, call(ws_bytes=need - 1), pre, b"workspace too small")


def test_bias_grad_argument_errors():
    lib = _lib.load()
    pre = b"bias_grad:"

    def call(dz=P, ldz=768, db=P, rows=4, N=768, ws=P, ws_bytes=BIG):
        return lib.aaclip_bias_grad(dz, ldz, db, rows, N, ws, ws_bytes, None)

    for n in ("dz", "db", "ws"):
        assert failed(lib, call(**{n: None}), pre, b"null"), n
        assert failed(lib, call(**{n: P + 4}), pre, b"aligned"), n
    for kw in (dict(rows=0), dict(N=0), dict(rows=-1)):
        assert failed(lib, call(**kw), pre, b"empty"), kw
    assert failed(lib, call(ldz=767), pre, b"ldz")
    assert failed(lib, call(ws_bytes=lib.aaclip_bias_grad_workspace_bytes(4, 768) - 1), pre, b"workspace too small")


def test_act_backward_argument_errors():
    lib = _lib.load()
    pre = b"act_backward:"

    def call(act=QB.GELU, zy=P, d_y=P, d_z=P, n=4096):
        return lib.aaclip_act_backward(act, zy, d_y, d_z, n, None)

    for act in (-1, 0, 1, 4):
        assert failed(lib, call(act=act), pre, b"activation"), act
    for n in ("zy", "d_y", "d_z"):
        assert failed(lib, call(**{n: None}), pre, b"null"), n
        assert failed(lib, call(**{n: P + 4}), pre, b"aligned"), n
    assert failed(lib, call(n=0), pre, b"empty") and failed(lib, call(n=-5), pre, b"empty")


def test_linear_smallk_backward_argument_errors():
    lib = _lib.load()
    pre = b"linear_smallk_backward:"

    def call(x=P, d_y=P, d_w=P, d_b=P, R=1536, N=768, K=2, ws=P, ws_bytes=BIG):
        return lib.aaclip_linear_smallk_backward(x, d_y, d_w, d_b, R, N, K, ws, ws_bytes, None)

    for n in ("x", "d_y", "ws"):
        assert failed(lib, call(**{n: None}), pre, b"null"), n
    assert failed(lib, call(d_w=None, d_b=None), pre, b"both NULL")
    for n in ("x", "d_y", "d_w", "d_b", "ws"):
        assert failed(lib, call(**{n: P + 4}), pre, b"aligned"), n
    for kw in (dict(R=0), dict(N=0), dict(K=0), dict(R=-1)):
        assert failed(lib, call(**kw), pre, b"empty"), kw
    assert failed(lib, call(K=5), pre, b"in_features")
    need = lib.aaclip_linear_smallk_backward_workspace_bytes(1536, 768, 2)
    assert failed(lib, call(ws_bytes=need - 1), pre, b"workspace too small")


@pytest.mark.parametrize("entry,name", QB.ALL_CASES)
def test_cases_are_well_conditioned(entry, name):
    """fp32 CPU autograd of the reference stays within 2.5e-5 of fp64 on every case: what makes the GPU bar of 1e-4
    attainable on these inputs."""
    table, inputs, reference, case = QB.ENTRIES[entry]
    t, want = case(name)
    got = reference(t, table[name], torch.float32)
    errs = {}
    for k, w in want.items():
        if w is None:
            continue
        if float(w.norm()) == 0:
            assert not got[k].any(), k
        else:
            errs[k] = rel(got[k], w)
    print(entry, name, errs)
    assert all(v <= 2.5e-5 for v in errs.values()), errs


def test_case_properties():
    t, want = QB.attention_case("one_key")
    assert not want["d_q"].any() and not want["d_k"].any() and want["d_v"].any()
    c = QB.ATTENTION["peaked_row"]
    p = QB.attention_reference(QB.attention_inputs("peaked_row"), c)["p"]        # [B, H, nq, Lk]
    assert float(p[:, :, 0].amax(-1).median()) > 0.9            # query 0: one key holds most of the mass
    assert float(p[:, :, 0].amin(-1).max()) < 1e-30             # and the far keys underflow towards zero
    assert QB.ATTENTION["production"] == dict(B=2, nq=2, Lk=2, H=8, hd=96)
    for name in ("d_q_only", "d_k_only", "d_v_only"):
        assert sum(w is not None for w in QB.attention_case(name)[1].values()) == 1
    for name, c in QB.BIAS.items():
        dz = QB.bias_case(name)[0]["dz"]
        assert dz.shape[1] == c["N"] + c["pad"] and bool(dz[:, c["N"]:].isnan().all()) and not dz[:, :c["N"]].isnan().any()
    for name, c in QB.ACT.items():
        z = QB.act_case(name)[0]["zy"]
        assert (z == 0).any()
        if c["n"] >= 255:
            assert (z == 10).any() and ((z == -10).any() or c["act"] == QB.RELU)
        if c["act"] == QB.RELU:
            assert (z >= 0).all()
    assert QB.chunks_of(2 * 768 + 3) == 49 and QB.chunks_of(1) == 1 and QB.chunks_of(10 ** 6) == QB.MAX_CHUNKS


# ---------------------------------------------------------------------------------------------- train.py
def test_stage2_loss_with_given_queries_is_unchanged():
    import head_backward_cases as HB
    import iqm_loss_cases as IC
    import train
    import visual_backward_cases as VB
    assert inspect.signature(train.stage2_loss).parameters["iqm_queries"].default is None
    model = HB.build_heads_model(torch.device("cpu"), "fp32")[3]
    image, mask, anchors, label = HB.heads_inputs()
    args = (model, image, mask.float(), label, anchors.float(), VB.TAPS_IMAGE)
    for shape in ((VB.TAPS_BATCH, 2, 512), (VB.TAPS_BATCH, 3, 256), (2, 256)):
        with pytest.raises(ValueError, match="iqm_queries"):
            train.stage2_loss(*args, torch.zeros(shape))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        train.stage2_loss(*args, IC.stage2_queries())
    with pytest.raises(ValueError, match="iqm_queries"):        # the branch is 768 wide, the seg tokens 256
        train.stage2_loss(*args)


def test_iqm_queries_refuses_levels_that_stop_short():
    class Stub:
        pass
    model = Stub()
    model.image_encoder = Stub()
    model.image_encoder.transformer = Stub()
    model.image_encoder.transformer.resblocks = [None] * 4
    model.levels = [1, 3]
    with pytest.raises(NotImplementedError, match="last block"):
        autograd.iqm_queries(model, [], None)
    with pytest.raises(NotImplementedError, match="last block"):
        autograd.visual_outputs(model, None, None)


class _Recorder:
    def __init__(self):
        self.calls = []


def test_train_image_adapter_call_order_and_checkpoint(tmp_path, monkeypatch):
    import train
    rec = _Recorder()

    class StubModel(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.image_adapter = torch.nn.ModuleDict({"seg_proj": torch.nn.Linear(2, 2)})
            for n in train.IQM_BRANCH_MODULES:
                setattr(self, n, torch.nn.Linear(2, 3))

    class StubLoss:
        def __init__(self, v):
            self.v = v

        def backward(self):
            rec.calls.append("backward")

        def item(self):
            return self.v

    class StubOpt:
        def zero_grad(self):
            rec.calls.append("zero_grad")

        def step(self):
            rec.calls.append("step")

        def state_dict(self):
            return {"stub": 1}

    class StubSched:
        def step(self):
            rec.calls.append("sched")

    seen = []

    def fake_loss(model, image, mask, label, anchors, img_size, iqm_queries=None):
        assert iqm_queries is None
        seen.append((tuple(image.shape), tuple(anchors.shape), img_size))
        rec.calls.append("loss")
        return StubLoss(float(len(seen)))

    monkeypatch.setattr(train, "stage2_loss", fake_loss)
    emb = {"a": torch.zeros(4, 2), "b": torch.ones(4, 2)}
    batches = [{"image": torch.zeros(2, 3, 8, 8), "mask": torch.zeros(2, 1, 8, 8), "label": torch.zeros(2, dtype=torch.long),
                "class_name": ["a", "b"]}] * 2
    model = StubModel()
    out = train.train_image_adapter(model, emb, batches, StubOpt(), StubSched(), "cpu", 1, str(tmp_path / "ckpt"), 3, 8,
                                    logging.getLogger("test"))
    assert out is model
    per_batch = ["loss", "zero_grad", "backward", "step", "sched"]
    assert rec.calls == per_batch * 4                                   # epochs 1 and 2, two batches each
    assert seen[0] == ((2, 3, 8, 8), (2, 4, 2), 8)
    assert sorted(os.listdir(tmp_path / "ckpt")) == ["image_adapter.pth", "image_adapter_2.pth", "image_adapter_3.pth"]
    last = torch.load(tmp_path / "ckpt" / "image_adapter.pth")
    assert set(last) == {"epoch", "image_adapter", "image_optimizer", "iqm_branch"} and last["epoch"] == 3
    assert set(last["iqm_branch"]) == set(train.IQM_BRANCH_MODULES)
    assert torch.load(tmp_path / "ckpt" / "image_adapter_2.pth")["epoch"] == 2
    assert torch.equal(last["image_adapter"]["seg_proj.weight"], model.image_adapter["seg_proj"].weight)
    fresh = StubModel()
    train.load_iqm_branch_state(fresh, last["iqm_branch"])
    assert torch.equal(fresh.iqm.weight, model.iqm.weight)
    assert "iqm_branch" in train.train_image_adapter.__doc__


# ---------------------------------------------------------------------------------------------- one forward, with a record
# Calls per engine function at the parent commit (060b204), counted with the stand-ins of engine_standins.py on the
# inputs of iqm_inputs() / branch_stub() below, its model/iqm.py, model/adapter.py and aaclip_hip/autograd.py run from a
# scratch copy of `git show`: IQM.forward; IqmQueries.forward (driven with a stub ctx and the stub model); and the calls
# AdaptedCLIP._iqm_branch makes outside IQM.forward (its total minus IQM.forward's on the same tensors).
# Per layer: 16 gemm at inference (self-attention 4, visual cross-attention 6, text cross-attention 4, feed-forward 2) and
# a 17th with a record, the pre-GELU rows; the text rows are fp32 here, so both cross-attentions are on cross_rows.
PARENT_IQM_FORWARD = {"gemm": 32, "head_expand": 4, "head_diag": 4, "cross_rows": 4, "small_attention": 2,
                      "residual_layernorm": 9, "combine3": 2}
PARENT_IQM_QUERIES_FORWARD = {"gemm": 36, "head_expand": 4, "head_diag": 4, "cross_rows": 4, "small_attention": 2,
                              "residual_layernorm": 10, "combine3": 3, "linear_smallk": 1}
PARENT_BRANCH_OUTSIDE_IQM = {"gemm": 2, "residual_layernorm": 1, "combine3": 1, "linear_smallk": 1}
IQM_LAYERS, IQM_HID, IQM_HEADS, IQM_B, IQM_LV, IQM_LT = 2, 256, 4, 2, 24, 11


def build_iqm(seed=5, text_width=IQM_HID):
    from model.iqm import IQM
    torch.manual_seed(seed)
    iqm = IQM(hidden_size=IQM_HID, num_hidden_layers=IQM_LAYERS, num_attention_heads=IQM_HEADS,
              encoder_hidden_size=IQM_HID, text_encoder_hidden_size=text_width, intermediate_size=64)
    with torch.no_grad():
        for p in iqm.parameters():
            p.normal_(0, 0.1 if p.dim() > 1 else 0.3)
        for m in iqm.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.add_(1.0)
    return iqm


def iqm_inputs():
    """IQM.forward's arguments: queries [2, 2, 256], visual rows [2, 24, 256] with an encoder_proj, text rows
    [2, 11, 256], fp32"""
    g = torch.Generator().manual_seed(6)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(query_embeds=r(IQM_B, 2, IQM_HID), query_length=2, encoder_hidden_states=r(IQM_B, IQM_LV, IQM_HID),
                text_encoder_hidden_states=r(IQM_B, IQM_LT, IQM_HID) * 0.7, code=_lib.F32,
                encoder_proj=(r(IQM_HID, IQM_HID) * 0.1, r(IQM_HID) * 0.2))


def record_keys(layers, branch):
    """The key set IQM.forward documents (branch: with the four AdaptedCLIP._iqm_branch adds)"""
    keys = {"vis", "txt", "last"} | ({"cls", "t1", "query", "te"} if branch else set())
    for l in range(layers):
        keys |= {f"{l}.{k}" for k in ("h", "a", "c", "mix", "z", "inter", "dense")}
        keys |= {f"{l}.a.{k}" for k in ("ctx", "dense", "q", "k", "v")}
        keys |= {f"{l}.c.{k}" for k in ("ctx", "dense", "qm", "qt", "ebar", "qx", "xbar")}
        keys |= {f"{l}.t.{k}" for k in ("ctx", "dense", "qm", "qt", "ebar")}
    return keys


def branch_stub():
    """The least of an AdaptedCLIP that its _iqm_branch and IqmQueries.forward read, and their inputs (rows, tap, anchors)"""
    from model.adapter import AdaptedCLIP

    class Stub(torch.nn.Module):
        _iqm_branch = AdaptedCLIP._iqm_branch

        def __init__(self):
            super().__init__()
            self.iqm, self.iqm_hidden_size, self.relu = build_iqm(), IQM_HID, False
            self.class_query_mlp = torch.nn.Sequential(torch.nn.Linear(32, IQM_HID), torch.nn.ReLU(),
                                                       torch.nn.Linear(IQM_HID, IQM_HID))
            self.visual_feature_proj = torch.nn.Linear(IQM_HID, IQM_HID)
            self.text_feature_proj = torch.nn.Linear(2, IQM_HID)
            self.pos_embedding = torch.nn.Parameter(torch.randn(1, 8, IQM_HID) * 0.1)
            self.iqm_layer_norm = torch.nn.LayerNorm(IQM_HID)

        def _code(self):
            return _lib.F32

    g = torch.Generator().manual_seed(8)
    return (Stub(), torch.randn(IQM_B, IQM_LV, IQM_HID, generator=g), torch.randn(IQM_B, 5, 32, generator=g),
            torch.randn(IQM_B, IQM_LT, 2, generator=g))


class StubCtx:
    def save_for_backward(self, *tensors):
        self.saved = tensors


def test_iqm_forward_with_and_without_a_record(monkeypatch):
    """One IQM.forward serves inference and training: a record changes neither the output nor the launches (but for the
    one product of the pre-GELU rows per layer), holds exactly the documented keys, and nothing is launched before the
    cases without a backward are refused."""
    import engine_standins as SI
    iqm, kw = build_iqm(), iqm_inputs()
    plain, rec, S = {}, {}, {}
    with torch.no_grad():
        SI.install(monkeypatch, plain)
        want = iqm(**kw).last_hidden_state
        SI.install(monkeypatch, rec)
        got = iqm(**kw, record=S).last_hidden_state
    assert plain.pop("require_gpu") == 1 and rec.pop("require_gpu") == 1
    assert torch.equal(got, want) and float(want.abs().max()) > 0.5
    assert set(S) == record_keys(IQM_LAYERS, branch=False)
    for k, t in S.items():
        assert t.dtype == (engine.torch_dtype(kw["code"]) if k in ("vis", "txt") else torch.float32), k
    assert S["0.c.qm"].shape == (IQM_B * 2 * IQM_HEADS, IQM_HID) and S["1.z"].shape == (IQM_B * 2, 64)
    assert plain == PARENT_IQM_FORWARD
    want_rec = {k: v - PARENT_BRANCH_OUTSIDE_IQM.get(k, 0) for k, v in PARENT_IQM_QUERIES_FORWARD.items()}
    assert rec == {k: v for k, v in want_rec.items() if v}
    assert {k: rec[k] - plain[k] for k in rec} == dict.fromkeys(rec, 0) | {"gemm": IQM_LAYERS}
    # the cases the backward does not cover: refused before anything runs
    none = {}
    SI.install(monkeypatch, none)
    lv = {"rows": [torch.zeros(IQM_B * 5, 32)], "rows_per_image": 5, "row0": 1, "keys": 4, "width": 32,
          "w_in": torch.zeros(32, IQM_HID), "w_out": torch.zeros(IQM_HID, 32)}
    with pytest.raises(NotImplementedError):
        iqm(**{**kw, "encoder_hidden_states": None}, encoder_levels=lv, record={})
    assert none == {}
    narrow = dict(kw, text_encoder_hidden_states=torch.zeros(IQM_B, IQM_LT, 64))     # no aaclip_cross_rows width
    iq2 = build_iqm(text_width=64)
    with torch.no_grad():
        assert iq2(**narrow).last_hidden_state.shape == (IQM_B, 2, IQM_HID)          # inference: the small_attention path
        assert none.get("small_attention", 0) > IQM_LAYERS
        with pytest.raises(NotImplementedError):
            iq2(**narrow, record={})


def test_iqm_queries_forward_is_the_models_branch(monkeypatch):
    """IqmQueries.forward is a caller of AdaptedCLIP._iqm_branch: the queries of the model's own call, the whole record
    saved, and the launches IqmQueries.forward made when it carried its own copy of the branch."""
    import engine_standins as SI
    model, rows, tap, anchors = branch_stub()
    counts, ctx = {}, StubCtx()
    with torch.no_grad():
        SI.install(monkeypatch)
        want = model._iqm_branch(tap, rows, anchors, IQM_B, tap.shape[1], _lib.F32).last_hidden_state
        SI.install(monkeypatch, counts)
        got = autograd.IqmQueries.forward(ctx, model, rows, tap, anchors)
    assert torch.equal(got, want) and got.shape == (IQM_B, 2, IQM_HID)
    assert set(ctx.keys) == record_keys(IQM_LAYERS, branch=True) and len(ctx.saved) == len(ctx.keys)
    assert ctx.dims == (IQM_B, tap.shape[1], IQM_LV, IQM_LT, _lib.F32)
    S = dict(zip(ctx.keys, ctx.saved))
    assert all(t.dtype == torch.float32 for t in S.values())
    assert S["vis"].data_ptr() == rows.data_ptr() and torch.equal(S["te"], anchors)
    assert torch.equal(S["cls"], tap[:, 0, :]) and bool((S["t1"] >= 0).all()) and bool((S["t1"] == 0).any())
    counts.pop("require_gpu")
    assert counts == PARENT_IQM_QUERIES_FORWARD
    with pytest.raises(NotImplementedError, match="text_embeddings"):
        autograd.IqmQueries.forward(StubCtx(), model, rows, tap, anchors[:, :, :1])
