"""CPU side of the IQM query-side backward: the new symbols and their signatures, the Python surface, the workspace
sizes, every device-free argument error of every new entry, the conditioning of the cases (fp32 CPU autograd against
fp64), stage2_loss with given queries, and train_image_adapter's call order and checkpoint with a stub model and loss."""
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
    assert in_header == 9 and lib.aaclip_version() == 9 and _lib.ABI_VERSION == 9
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
