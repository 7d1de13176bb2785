"""CPU side of the IQM map term of the stage-2 loss (aaclip_iqm_map_train and its backward): the symbols and the ABI
number, the Python surface, the device-free argument errors, the backward's step sequence and its support windows
against fp64 autograd, and the conditioning of the cases."""
import os
import re

import numpy as np
import pytest
import torch

import head_backward_cases as HB
import iqm_loss_cases as IC
import visual_backward_cases as VB
from aaclip_hip import _lib, autograd, engine
from conftest import REPO
from visual_backward_cases import rel

SYMBOLS = ("aaclip_iqm_map_train", "aaclip_iqm_map_train_backward_workspace_bytes", "aaclip_iqm_map_train_backward")
P = 0x7f0000001000      # a plausible, 16-byte aligned device address: nothing here may be dereferenced
BIG = 1 << 40


def test_symbols_and_abi_version():
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "aaclip.h")).read()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
        assert re.search(r"\b%s\(" % name, header)
    in_header = int(re.search(r"#define\s+AACLIP_ABI_VERSION\s+(\d+)", header).group(1))
    assert in_header == 10 and lib.aaclip_version() == 10 and _lib.ABI_VERSION == 10


def test_python_surface():
    import train
    assert hasattr(engine, "iqm_map_train") and hasattr(engine, "iqm_map_train_backward")
    assert hasattr(autograd, "IqmMapTrain") and hasattr(autograd, "iqm_map_train")
    assert hasattr(train, "stage2_loss") and train.IQM_WEIGHT == 0.4
    assert train.TEXT_WEIGHT + train.IQM_WEIGHT == 1.0
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.iqm_map_train(torch.zeros(1, 4, 256), torch.zeros(1, 2, 256), 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.iqm_map_train_backward(torch.zeros(1, 4, 256), torch.zeros(1, 2, 256), torch.zeros(1, 4),
                                      torch.zeros(1, 2, 8, 8))


def test_query_width_mismatch_raises_before_any_gpu_work():
    """With CPU tensors the first piece of GPU work raises RuntimeError; a wrong query width must raise ValueError."""
    import train
    model = HB.build_heads_model(torch.device("cpu"), "fp32")[3]
    image, mask, anchors, label = HB.heads_inputs()
    args = (model, image, mask.float(), label, anchors.float(), VB.TAPS_IMAGE)
    for shape in ((VB.TAPS_BATCH, 2, 512), (VB.TAPS_BATCH, 2, 128), (VB.TAPS_BATCH, 3, 256), (2, 256)):
        with pytest.raises(ValueError, match="iqm_queries"):
            train.stage2_loss(*args, torch.zeros(shape))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        train.stage2_loss(*args, IC.stage2_queries())


# ---------------------------------------------------------------------------------------------- argument checks
def fwd(lib, seg=P, q=P, grid=P, out=P, B=2, g=37, E=768, S=518):
    return lib.aaclip_iqm_map_train(seg, q, grid, out, B, g, E, S, None)


def bwd(lib, seg=P, q=P, grid=P, d_preds=P, d_seg=P, d_q=P, B=2, g=37, E=768, S=518, ws=P, ws_bytes=BIG):
    return lib.aaclip_iqm_map_train_backward(seg, q, grid, d_preds, d_seg, d_q, B, g, E, S, ws, ws_bytes, None)


def test_argument_errors():
    lib = _lib.load()

    def failed(rc, word, prefix):
        msg = lib.aaclip_last_error()
        return rc < 0 and word in msg and (msg.startswith(prefix) or word == b"row width")

    for call, prefix, names in ((fwd, b"iqm_map_train:", ("seg", "q", "grid", "out")),
                                (bwd, b"iqm_map_train_backward:", ("seg", "q", "grid", "d_preds", "ws"))):
        for n in names:
            assert failed(call(lib, **{n: None}), b"null", prefix), n
        for n in names + (("d_seg", "d_q") if call is bwd else ()):
            assert failed(call(lib, **{n: P + 4}), b"aligned", prefix), n
        assert failed(call(lib, E=100), b"row width", prefix)
        for bad in ({"g": 41}, {"g": 0}, {"S": 2049}, {"S": 0}, {"B": 0}, {"B": 65536}):
            assert failed(call(lib, **bad), b"shape", prefix), bad
    assert failed(bwd(lib, d_seg=None, d_q=None), b"nothing to compute", b"iqm_map_train_backward:")
    need = lib.aaclip_iqm_map_train_backward_workspace_bytes(2, 37, 768, 518)
    assert failed(bwd(lib, ws_bytes=need - 1), b"workspace too small", b"iqm_map_train_backward:")
    q = lib.aaclip_iqm_map_train_backward_workspace_bytes
    assert q(0, 37, 768, 518) == 0 and q(2, 0, 768, 518) == 0 and q(2, 37, 0, 518) == 0 and q(2, 37, 768, 0) == 0
    # T [B, S, g], dz and four scalars per patch, the chunked query sums
    assert need >= (2 * 518 * 37 + 5 * 2 * 1369 + 2 * 2 * 768) * 4


@pytest.mark.parametrize("ptrs", [{}, {"d_seg": None}, {"d_q": None}])
def test_valid_calls_pass_every_check_up_to_the_workspace(ptrs):
    """A valid call with a 16-byte workspace fails on the workspace size and on nothing before it: that check is the
    last one in front of the first launch."""
    lib = _lib.load()
    for B, g, S, E, _, _ in IC.IQM_CASES.values():
        rc = bwd(lib, B=B, g=g, E=E, S=S, ws_bytes=16, **ptrs)
        assert rc < 0 and b"workspace too small" in lib.aaclip_last_error(), lib.aaclip_last_error()


# ---------------------------------------------------------------------------------------------- the backward's steps
def step_sequence(name, ft):
    """Steps 1-5 of the backward as csrc/iqm_loss.hip runs them, in fp64 torch, with the half-pixel weights and support
    windows of the numpy mirror evaluated in `ft` -> (d_seg, d_queries)"""
    B, g, S, E, _, _ = IC.IQM_CASES[name]
    t, want = IC.iqm_case(name)
    f, q, dP = t["seg"].double(), t["queries"].double(), want["d_preds"].double()
    q0, q1 = q[:, 0:1], q[:, 1:2]
    ff, n0, n1 = (f * f).sum(-1), (q0 * q0).sum(-1), (q1 * q1).sum(-1)
    c0, c1 = (f * q0).sum(-1) / (ff * n0).sqrt(), (f * q1).sum(-1) / (ff * n1).sqrt()
    p = torch.sigmoid(c1 - c0)
    dU = dP[:, 1] - dP[:, 0]                                          # 1
    W = torch.from_numpy(IC.hp_matrix(g, S, ft))                      # 2: fine columns, then fine rows
    T = dU @ W
    dgrid = torch.einsum("yc,byx->bcx", W, T).reshape(B, g * g)
    dz = p * (1 - p) * dgrid                                          # 3
    nf = ff.sqrt()
    d_seg = dz.unsqueeze(-1) * ((q1 / (nf * n1.sqrt()).unsqueeze(-1) - (c1 / ff).unsqueeze(-1) * f)      # 4
                                - (q0 / (nf * n0.sqrt()).unsqueeze(-1) - (c0 / ff).unsqueeze(-1) * f))
    a = ((dz / nf).unsqueeze(-1) * f).sum(1)                          # 5
    d_q1 = a / n1.sqrt() - (dz * c1).sum(1, keepdim=True) * q1[:, 0] / n1
    d_q0 = -(a / n0.sqrt() - (dz * c0).sum(1, keepdim=True) * q0[:, 0] / n0)
    return d_seg, torch.stack([d_q0, d_q1], dim=1)


@pytest.mark.parametrize("name", list(IC.IQM_CASES))
def test_step_sequence_is_the_gradient(name):
    """With the mirror evaluated in fp64 (torch's own arithmetic for the weights) the steps reproduce fp64 autograd to
    1e-12; in float32, the kernels' arithmetic, a weight moves by at most g 2^-22 (the rounding of scale (y + 0.5) -
    0.5, a value below g).  What that costs the gradients is printed."""
    B, g, S, E, _, _ = IC.IQM_CASES[name]
    want = IC.iqm_case(name)[1]
    d_seg, d_q = step_sequence(name, np.float64)
    errs = {"d_seg": rel(d_seg, want["d_seg"]), "d_queries": rel(d_q, want["d_queries"])}
    print(name, errs)
    assert all(v <= 1e-12 for v in errs.values()), errs
    dw = np.abs(IC.hp_matrix(g, S, np.float32) - IC.hp_matrix(g, S, np.float64)).max()
    assert dw <= g * 2.0 ** -22, dw
    d_seg, d_q = step_sequence(name, np.float32)
    errs32 = {"d_seg": rel(d_seg, want["d_seg"]), "d_queries": rel(d_q, want["d_queries"])}
    print(name, "float32 weights", errs32)


def test_support_windows_hold_every_weight():
    """float32 mirror: every (fine, coarse) pair with a non-zero forward weight lies inside the coarse index's support
    window, and the weights of every fine index sum to 1."""
    for g in range(1, 41):
        for S in sorted({1, 2, g - 1, g, g + 1, 33, 70, 518, 2048} - {0}):
            win = [IC.hp_support(c, g, S) for c in range(g)]
            for lo, hi in win:
                assert 0 <= lo <= hi <= S - 1, (g, S, lo, hi)
            for y in range(S):
                i0, i1, l0, l1 = IC.hp_source(y, g, S)
                assert 0 <= i0 <= i1 <= g - 1 and i1 - i0 <= 1, (g, S, y)
                assert abs(float(l0) + float(l1) - 1.0) <= 2.0 ** -23, (g, S, y)
                for i, l in ((i0, l0), (i1, l1)):
                    if l != 0:
                        assert win[i][0] <= y <= win[i][1], (g, S, y, i, win[i])
            if g > 1 and S >= g:       # the clamped edges: coarse 0 from fine 0 on, the last coarse index up to S - 1
                assert win[0][0] == 0 and win[g - 1][1] == S - 1


@pytest.mark.parametrize("name", list(IC.IQM_CASES))
def test_cases_are_well_conditioned(name):
    """The reference in fp32 torch on the CPU stays within 2.5e-5 relative Frobenius of fp64, so the GPU bar of 1e-4
    leaves a 4x margin over plain fp32."""
    want = IC.iqm_case(name)[1]
    got = IC.iqm_reference(name, torch.float32)
    errs = {k: rel(got[k], want[k]) for k in ("map", "d_seg", "d_queries")}
    print(name, errs)
    assert all(v <= 2.5e-5 for v in errs.values()), errs


def test_subset_queries_span_the_sigmoid():
    spans = {}
    for name, c in IC.IQM_CASES.items():
        p = IC.iqm_case(name)[1]["p"]
        spans[name] = (float(p.min()), float(p.max()))
        if c[4] == IC.SUBSETS:
            assert spans[name][0] <= 0.3 and spans[name][1] >= 0.7, spans
    assert sum(c[4] == IC.SUBSETS for c in IC.IQM_CASES.values()) >= 2
    print(spans)
