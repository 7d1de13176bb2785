"""The bf16x3 backward without a GPU: engine.split3_weight, the C ABI's new symbols and their binding, the
AACLIP_BACKWARD switch, and the preconditions of tests/test_gpu_backward_bf16x3.py -- the arithmetic's own emulation
stays inside the bar on every attention case that file runs, and the adapter case keeps clear of the LeakyReLU kink."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import backward_bf16x3_cases as BC
from aaclip_hip import _lib, autograd, engine
from conftest import PKG

NEW_SYMBOLS = ("aaclip_split3_rows", "aaclip_attention_backward_long_bf16x3_workspace_bytes",
               "aaclip_attention_backward_long_bf16x3", "aaclip_block_backward_long_bf16x3_workspace_bytes",
               "aaclip_block_backward_long_bf16x3")


# ---------------------------------------------------------------------------------------------- split3_weight
def test_split3_weight_layout_and_precision():
    N, K = 96, 64
    w = BC.rnd("bf16x3.weight", (N, K)) * torch.logspace(-12, 6, N).reshape(N, 1)
    s = engine.split3_weight(w)
    assert s.dtype == torch.bfloat16 and s.shape == (N, 3 * K) and s.is_contiguous()
    hi, hi2, lo = s[:, :K], s[:, K:2 * K], s[:, 2 * K:]
    assert torch.equal(hi, w.bfloat16()) and torch.equal(hi2, hi)
    assert torch.equal(lo, (w - hi.float()).bfloat16())
    err = ((hi.double() + lo.double()) - w.double()).abs()
    assert bool((err <= 2.0 ** -17 * w.double().abs()).all()), float((err / w.double().abs()).max())


def test_split3_weight_scales_the_q_rows_exactly():
    D = 64
    w = BC.rnd("bf16x3.weight.q", (3 * D, D))
    s, plain = engine.split3_weight(w, q_rows=D), engine.split3_weight(w)
    assert torch.equal(s[:D].float(), plain[:D].float() * 0.125)          # a power of two: the planes scale exactly
    assert torch.equal(s[D:], plain[D:])
    assert torch.equal(w, BC.rnd("bf16x3.weight.q", (3 * D, D)))           # the argument is left alone


def test_weight_cache_kinds_follow_the_parameter_version():
    D = 64
    p = torch.nn.Parameter(BC.rnd("bf16x3.weight.cache", (3 * D, D)))
    b = torch.nn.Parameter(BC.rnd("bf16x3.bias.cache", (3 * D,)))
    cache = engine.WeightCache()
    first = {k: cache.get(p, engine.BF16, k) for k in ("split3", "split3_t", "split3_q")}
    assert torch.equal(first["split3"], engine.split3_weight(p))
    assert torch.equal(first["split3_t"], engine.split3_weight(p.detach().t())) and first["split3_t"].shape == (D, 9 * D)
    assert torch.equal(first["split3_q"], engine.split3_weight(p, q_rows=D))
    sb = cache.get(b, engine.F32, "scale_q")
    assert torch.equal(sb[:D], b.detach()[:D] * 0.125) and torch.equal(sb[D:], b.detach()[D:])
    assert cache.get(p, engine.BF16, "split3") is first["split3"]
    with torch.no_grad():
        p.mul_(2.0)
    assert torch.equal(cache.get(p, engine.BF16, "split3_q"), engine.split3_weight(p, q_rows=D))
    assert not torch.equal(cache.get(p, engine.BF16, "split3"), first["split3"])


# ---------------------------------------------------------------------------------------------- the C ABI
def test_library_exports_the_new_symbols():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert _lib.load().aaclip_version() == 10 == _lib.ABI_VERSION
    with open(os.path.join(os.path.dirname(PKG), "include", "aaclip.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
    assert "#define AACLIP_ABI_VERSION 10 " in header


def test_workspace_sizes():
    lib = _lib.load()
    a = lib.aaclip_attention_backward_long_bf16x3_workspace_bytes
    assert a(0, 5, 5) == 0 and a(2, 1370, 16) >= a(2, 1369, 16) > 8 * 2 * 16 * 1369 * 128
    assert a(2, 1370, 16) >= lib.aaclip_attention_backward_long_workspace_bytes(2, 1370, 16) + 8 * 2 * 16 * 1370 * 128
    b = lib.aaclip_block_backward_long_bf16x3_workspace_bytes
    assert b(0, 5, 256, 1024) == 0
    # the fp32 layout (which already holds the statistics) + one split3 buffer [rows, 3F] + the eight planes
    assert b(2, 170, 1024, 4096) >= (lib.aaclip_block_backward_long_workspace_bytes(2, 170, 1024, 4096)
                                     + 340 * 3 * 4096 * 2 + 8 * 2 * 16 * 170 * 128)


# ---------------------------------------------------------------------------------------------- the switch
def test_backward_precision_switch():
    before = autograd.backward_precision()
    assert before in engine.BACKWARD_PRECISIONS
    with autograd.use_backward_precision("bf16x3"):
        assert autograd.backward_precision() == "bf16x3"
        with autograd.use_backward_precision("fp32"):
            assert autograd.backward_precision() == "fp32"
        assert autograd.backward_precision() == "bf16x3"
    assert autograd.backward_precision() == before
    with pytest.raises(ValueError, match="bf16x3"):
        autograd.set_backward_precision("bf16")
    with pytest.raises(ValueError):
        with autograd.use_backward_precision("fp16x2"):
            pass
    assert autograd.backward_precision() == before
    with pytest.raises(RuntimeError):             # an exception inside the block still restores the mode
        with autograd.use_backward_precision("bf16x3"):
            raise RuntimeError("x")
    assert autograd.backward_precision() == before


def test_environment_variable_parsing():
    assert autograd.backward_precision_from_env({}) == "fp32"
    assert autograd.backward_precision_from_env({"AACLIP_BACKWARD": ""}) == "fp32"
    assert autograd.backward_precision_from_env({"AACLIP_BACKWARD": "fp32"}) == "fp32"
    assert autograd.backward_precision_from_env({"AACLIP_BACKWARD": "bf16x3"}) == "bf16x3"
    for bad in ("bf16", "fp16x2", "1"):
        with pytest.raises(ValueError, match="bf16x3"):
            autograd.backward_precision_from_env({"AACLIP_BACKWARD": bad})


@pytest.mark.parametrize("value,want", [("bf16x3", "mode=bf16x3"), ("bf16", "ValueError")])
def test_environment_variable_sets_the_initial_mode(value, want):
    """AACLIP_BACKWARD is read when aaclip_hip.autograd is imported: a fresh interpreter"""
    env = dict(os.environ, AACLIP_BACKWARD=value)
    env["PYTHONPATH"] = os.pathsep.join([PKG] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    code = ("try:\n"
            "    from aaclip_hip import autograd\n"
            "    print('mode=' + autograd.backward_precision())\n"
            "except ValueError:\n"
            "    print('ValueError')\n")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout
    assert out.strip().splitlines()[-1] == want, out


def test_unknown_precision_is_refused_before_anything_else():
    x = torch.zeros(2, 192)
    with pytest.raises(ValueError, match="bf16x3"):
        engine.attention_backward(x, torch.zeros(2, 64), 1, 2, 1, False, precision="bf16")
    with pytest.raises(ValueError, match="bf16x3"):
        engine.block_backward(x, None, 1, 2, 1, x, precision="fp16x2")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.attention_backward(x, torch.zeros(2, 64), 1, 2, 1, False, precision="bf16x3")


# ---------------------------------------------------------------------------------------------- the GPU file's inputs
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("B,H,L", BC.ATTENTION_CASES)
def test_emulation_fits_the_bar(B, H, L, causal):
    qkv, d_ctx, want = BC.VB.attention_case(B, H, L, causal)
    errs = BC.attention_errors(BC.attention_backward_emulated(qkv, d_ctx, B, H, L, causal), want, H)
    print("emulated", B, H, L, causal, errs)
    assert all(v <= BC.BAR / 2 for v in errs.values()), errs       # measured: <= 1.5e-5


def test_emulation_fits_the_bar_on_peaked_rows():
    B, H, L, _ = BC.PEAKED
    qkv, d_ctx, want = BC.peaked_case()
    got = BC.attention_backward_emulated(qkv, d_ctx, B, H, L, False)
    errs = BC.attention_errors(got, want, H, rows=L)
    print("emulated peaked", errs)
    assert not got[L:].any()
    assert all(v <= BC.BAR / 2 for v in errs.values()), errs       # measured: 3.6e-5


def test_emulation_keeps_the_range():
    B, H, L, factor = BC.RANGE
    qkv, small, want = BC.range_case()
    errs = BC.attention_errors(BC.attention_backward_emulated(qkv, small, B, H, L, False), want, H)
    assert all(v <= BC.BAR / 2 for v in errs.values()), errs
    assert not small.half().any()                                   # what fp16 operands would see of this d_ctx


def test_adapter_case_keeps_clear_of_the_kink():
    z = BC.adapter_case()[7]
    clearance = float(z.abs().min() / z.pow(2).mean().sqrt())
    print("adapter case: min|z| / rms(z) =", clearance)
    assert clearance >= BC.Z_CLEARANCE, clearance                   # measured: 8.7e-4
