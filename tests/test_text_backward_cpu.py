"""CPU side of the text-tower backward: the yardstick (the oracle's fp64 autograd against what the reference's own
encode_text + loss chain gave, tests/golden/text_backward.npz), the device-free argument errors of the new entry points
(every check precedes the first HIP call) and the workspace query."""
import ctypes as C
import os

import numpy as np
import torch

import text_backward_cases as TB
from aaclip_hip import _lib, synth
from conftest import GOLDEN

P = 0x7f0000001000      # plausible, 16-byte aligned device addresses: nothing here may be dereferenced


def test_oracle_fp64_autograd_reproduces_reference_gradients():
    """Both sides are the same math in fp64 (the reference's modules under torch autograd; the oracle's straight-line
    restatement under torch autograd).  Measured when the record was generated: loss 2.0e-16 relative; the fp64 rows
    of the two gradients 3.5e-15 and 2.3e-15 relative Frobenius; the whole tensors against their fp32 copies 2.5e-8.
    Bars: 1e-12 for fp64 (sums of up to 1024 products in another order: ~1e3 x 1.1e-16, with a margin of 10 for
    cancellation) and 6e-8 = 2^-24 for the fp32 copies (half an ulp per stored element)."""
    g = np.load(os.path.join(GOLDEN, "text_backward.npz"))
    cfg = synth.tiny_cfg()
    sd = synth.synth_clip_state_dict(cfg, seed=7)
    ta = {k: v.double().requires_grad_(True)
          for k, v in synth.synth_text_adapter_state_dict(cfg, until=1, seed=7).items()}
    tok = torch.from_numpy(g["tokens"]).long()
    f, mask = TB.patch_inputs()
    loss = TB.oracle_loss(tok[0:1], tok[1:2], sd, ta, cfg.text.heads, 1, f, mask, TB.IMG, TB.NORM_WEIGHT, torch.float64)
    loss.backward()
    e_loss = abs(loss.item() - float(g["loss"])) / abs(float(g["loss"]))
    print("loss rel", e_loss)
    assert e_loss <= 1e-12
    assert set(ta) == {"0.fc.0.weight", "1.fc.0.weight"}
    for k, v in ta.items():
        r64 = torch.from_numpy(g["grad64." + k])
        r32 = torch.from_numpy(g["grad." + k]).double()
        e64 = float((v.grad[::TB.ROW_STEP] - r64).norm() / r64.norm())
        e32 = float((v.grad - r32).norm() / r32.norm())
        print(k, e64, e32)
        assert e64 <= 1e-12, (k, e64)
        assert e32 <= 6e-8, (k, e32)


def _err(lib):
    return lib.aaclip_last_error()


def test_workspace_query_is_monotonic_in_rows():
    lib = _lib.load()
    for D, F in ((256, 1024), (768, 3072), (1024, 4096)):
        prev = 0
        for rows in (1, 2, 77, 154, 1232, 4000, 4097, 4929, 19712):
            n = lib.aaclip_text_backward_workspace_bytes(rows, D, F)
            assert n > prev, (rows, D, F)
            prev = n
        # room for every recomputed row of a block: 7 D-wide, 2 3D-wide and 2 F-wide fp32 buffers
        assert prev >= 19712 * (7 * D + 6 * D + 2 * F) * 4
    assert lib.aaclip_text_backward_workspace_bytes(0, 768, 3072) == 0
    assert lib.aaclip_text_backward_workspace_bytes(77, 0, 3072) == 0


def test_gemm_wgrad_argument_errors():
    lib = _lib.load()
    big = 1 << 40
    assert lib.aaclip_gemm_wgrad(None, 256, P, 256, P, 77, 256, 256, P, big, None) < 0 and b"null" in _err(lib)
    assert lib.aaclip_gemm_wgrad(P, 256, P, 256, P, 0, 256, 256, P, big, None) < 0 and b"rows" in _err(lib)
    assert lib.aaclip_gemm_wgrad(P, 200, P, 256, P, 77, 200, 256, P, big, None) < 0 and b"128" in _err(lib)
    assert lib.aaclip_gemm_wgrad(P, 128, P, 256, P, 77, 256, 256, P, big, None) < 0 and b"stride" in _err(lib)
    assert lib.aaclip_gemm_wgrad(P + 4, 256, P, 256, P, 77, 256, 256, P, big, None) < 0 and b"aligned" in _err(lib)
    # 1232 rows are split into chunks: the partial products need a workspace
    assert lib.aaclip_gemm_wgrad(P, 768, P, 768, P, 1232, 768, 768, P, 1024, None) < 0 and b"workspace" in _err(lib)
    assert lib.aaclip_gemm_wgrad(P, 768, P, 768, P, 1232, 768, 768, None, 0, None) < 0 and b"workspace" in _err(lib)


def test_attention_backward_argument_errors():
    lib = _lib.load()
    assert lib.aaclip_attention_backward(None, P, P, 2, 77, 4, 1, 1.0, None) < 0 and b"null" in _err(lib)
    assert lib.aaclip_attention_backward(P, P, P, 2, 129, 4, 1, 1.0, None) < 0 and b"128" in _err(lib)
    assert lib.aaclip_attention_backward(P, P, P, 2, 1370, 16, 0, 1.0, None) < 0 and b"128" in _err(lib)
    assert lib.aaclip_attention_backward(P, P, P, 0, 77, 4, 1, 1.0, None) < 0 and b"empty" in _err(lib)
    assert lib.aaclip_attention_backward(P, P, P, 70000, 77, 4, 1, 1.0, None) < 0 and b"grid" in _err(lib)


def test_row_kernel_argument_errors():
    lib = _lib.load()
    assert lib.aaclip_layernorm_backward(P, P, None, None, P, 4, 256, 1e-5, None) < 0 and b"null" in _err(lib)
    assert lib.aaclip_layernorm_backward(P, P, P, None, P, 4, 300, 1e-5, None) < 0 and b"row width" in _err(lib)
    assert lib.aaclip_layernorm_backward(P, P, P, None, P, 0, 256, 1e-5, None) < 0 and b"rows" in _err(lib)
    assert lib.aaclip_adapter_mix_backward(P, P, P, None, P, 4, 256, 0.1, None) < 0 and b"null" in _err(lib)
    assert lib.aaclip_adapter_mix_backward(P, P, P, P, P, 4, 640, 0.1, None) < 0 and b"row width" in _err(lib)
    assert lib.aaclip_adapter_mix_backward(P, P, P, P, P, -1, 256, 0.1, None) < 0 and b"rows" in _err(lib)


def _weights(adapter=True):
    w = _lib.BlockWeights()
    for n, _ in _lib.BlockWeights._fields_[1:13]:
        setattr(w, n, P)
    if adapter:
        w.adapter_w = P
    return w


def test_block_backward_argument_errors():
    lib = _lib.load()
    big = 1 << 40

    def call(w, wt, B=2, L=77, D=256, H=4, F=1024, mode=1, d_in=P, d_aw=P, ws=P, ws_bytes=big, x=P):
        return lib.aaclip_block_backward(x, C.byref(w), C.byref(wt), 0.1, B, L, D, H, F, mode, P, d_in, d_aw, ws,
                                         ws_bytes, None)

    w, wt = _weights(), _weights()
    assert call(w, wt, x=None) < 0 and b"null" in _err(lib)
    old = _weights()
    old.struct_bytes = 13 * 8
    assert call(old, wt) < 0 and b"struct_bytes" in _err(lib)
    assert call(w, old) < 0 and b"struct_bytes" in _err(lib)
    assert call(w, wt, mode=2) < 0 and b"attn_mode" in _err(lib)
    assert call(w, wt, D=256, H=3) < 0 and b"64*H" in _err(lib)
    assert call(w, wt, D=320, H=5) < 0 and b"row width" in _err(lib)
    assert call(w, wt, F=1000) < 0 and b"multiple of 128" in _err(lib)
    assert call(w, wt, L=129) < 0 and b"128" in _err(lib)
    assert call(w, wt, L=1370, D=1024, H=16, F=4096, mode=0) < 0 and b"128" in _err(lib)
    assert call(w, wt, d_aw=None) < 0 and b"d_adapter_w" in _err(lib)
    assert call(_weights(False), wt, d_in=None) < 0 and b"nothing to compute" in _err(lib)
    assert call(w, _lib.BlockWeights()) < 0 and b"transposed" in _err(lib)
    need = lib.aaclip_text_backward_workspace_bytes(2 * 77, 256, 1024)
    assert call(w, wt, ws_bytes=need - 1) < 0 and b"workspace" in _err(lib)
    bad = _weights()
    bad.fc_w = None
    assert call(bad, wt) < 0 and b"null weight" in _err(lib)


def test_row_head_backward_argument_errors():
    lib = _lib.load()
    big = 1 << 40

    def call(x=P, tokens=P, pwt=P, act=1, d_x=P, d_w=P, n=2, T=77, D=256, E=256, mode=0, ws_bytes=big):
        return lib.aaclip_row_head_backward(x, tokens, P, P, P, pwt, act, P, d_x, d_w, n, T, D, E, mode, P, ws_bytes,
                                            None)

    assert call(x=None) < 0 and b"null" in _err(lib)
    assert call(d_w=None) < 0 and b"null" in _err(lib)
    assert call(tokens=None) < 0 and b"tokens" in _err(lib)
    assert call(pwt=None) < 0 and b"transposed" in _err(lib)
    assert call(mode=2) < 0 and b"mode" in _err(lib)
    assert call(act=3) < 0 and b"activation" in _err(lib)
    assert call(D=300) < 0 and b"row width" in _err(lib)
    assert call(E=200) < 0 and b"E must" in _err(lib)
    assert call(E=2048) < 0 and b"E must" in _err(lib)
    assert call(n=0) < 0 and b"shape" in _err(lib)
    assert call(ws_bytes=1024) < 0 and b"workspace" in _err(lib)
