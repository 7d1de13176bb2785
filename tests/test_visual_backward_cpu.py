"""CPU side of the long-row backward (aaclip_attention_backward_long, aaclip_block_backward_long): the symbols and the
ABI number, the device-free argument errors (every check precedes the first HIP call) and the workspace queries.  The
old entry points keep their 128-token limit."""
import ctypes as C
import os
import re

import visual_backward_cases as VB
from aaclip_hip import _lib
from conftest import REPO

P = 0x7f0000001000      # plausible, 16-byte aligned device addresses: nothing here may be dereferenced
BIG = 1 << 40


def _err(lib):
    return lib.aaclip_last_error()


def test_symbols_and_abi_version():
    lib = _lib.load()
    for name in ("aaclip_attention_backward_long_workspace_bytes", "aaclip_attention_backward_long",
                 "aaclip_block_backward_long_workspace_bytes", "aaclip_block_backward_long"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    header = open(os.path.join(REPO, "include", "aaclip.h")).read()
    in_header = int(re.search(r"#define\s+AACLIP_ABI_VERSION\s+(\d+)", header).group(1))
    assert in_header == 10 and lib.aaclip_version() == 10 and _lib.ABI_VERSION == 10


def test_attention_workspace_query():
    lib = _lib.load()
    q = lib.aaclip_attention_backward_long_workspace_bytes
    assert q(0, 1370, 16) == 0 and q(2, 0, 16) == 0 and q(2, 1370, 0) == 0
    prev = 0
    for L in (1, 31, 32, 77, 128, 129, 257, 1370, 5000):
        n = q(2, L, 16)
        assert n >= 3 * 2 * 16 * L * 4 and n >= prev, L          # the 3*B*H*L statistics
        prev = n
    assert q(3, 1370, 16) > q(2, 1370, 16) and q(2, 1370, 17) > q(2, 1370, 16) and q(2, 1371, 16) > q(2, 1370, 16)


def test_block_workspace_query():
    lib = _lib.load()
    q = lib.aaclip_block_backward_long_workspace_bytes
    assert q(0, 1370, 1024, 4096) == 0 and q(2, 0, 1024, 4096) == 0 and q(2, 1370, 0, 4096) == 0
    prev = 0
    for L in (1, 77, 128, 129, 170, 1370, 2740):
        n = q(2, L, 1024, 4096)
        assert n > prev, L
        prev = n
        # the text-backward layout for B*L rows plus the attention workspace
        assert n == (lib.aaclip_text_backward_workspace_bytes(2 * L, 1024, 4096)
                     + lib.aaclip_attention_backward_long_workspace_bytes(2, L, 16))


def test_attention_backward_long_argument_errors():
    lib = _lib.load()

    def call(qkv=P, d_ctx=P, d_qkv=P, B=2, L=VB.VISUAL_L, H=VB.VISUAL_H, ws=P, ws_bytes=BIG):
        return lib.aaclip_attention_backward_long(qkv, d_ctx, d_qkv, B, L, H, 0, 1.0, ws, ws_bytes, None)

    assert call(qkv=None) < 0 and b"null" in _err(lib)
    assert call(d_ctx=None) < 0 and b"null" in _err(lib)
    assert call(d_qkv=None) < 0 and b"null" in _err(lib)
    assert call(ws=None) < 0 and b"null" in _err(lib)
    assert call(B=0) < 0 and b"empty" in _err(lib)
    assert call(L=0) < 0 and b"empty" in _err(lib)
    assert call(H=0) < 0 and b"empty" in _err(lib)
    assert call(B=70000, L=77) < 0 and b"grid" in _err(lib)
    assert call(H=70000, L=77, B=1) < 0 and b"grid" in _err(lib)
    assert call(qkv=P + 4) < 0 and b"aligned" in _err(lib)
    assert call(d_ctx=P + 8) < 0 and b"aligned" in _err(lib)
    assert call(ws=P + 4) < 0 and b"aligned" in _err(lib)
    need = lib.aaclip_attention_backward_long_workspace_bytes(2, VB.VISUAL_L, VB.VISUAL_H)
    assert call(ws_bytes=need - 1) < 0 and b"workspace" in _err(lib)


def test_visual_length_passes_every_check_up_to_the_launch():
    """L = 1370, H = 16 with valid pointers fails on the short workspace and on nothing before it: the workspace check
    is the last one in front of the launch."""
    lib = _lib.load()
    for causal in (0, 1):
        for L in (129, VB.VISUAL_L):
            rc = lib.aaclip_attention_backward_long(P, P, P, 2, L, VB.VISUAL_H, causal, 0.125, P, 16, None)
            assert rc < 0 and b"workspace too small" in _err(lib), _err(lib)


def _weights(adapter=True):
    w = _lib.BlockWeights()
    for n, _ in _lib.BlockWeights._fields_[1:13]:
        setattr(w, n, P)
    if adapter:
        w.adapter_w = P
    return w


def test_block_backward_long_argument_errors():
    lib = _lib.load()

    def call(w, wt, B=2, L=1370, D=1024, H=16, F=4096, mode=0, d_in=P, d_aw=P, ws=P, ws_bytes=BIG, x=P):
        return lib.aaclip_block_backward_long(x, C.byref(w), C.byref(wt), 0.1, B, L, D, H, F, mode, P, d_in, d_aw, ws,
                                              ws_bytes, None)

    w, wt = _weights(), _weights()
    assert call(w, wt, x=None) < 0 and b"null" in _err(lib)
    assert call(w, wt, ws=None) < 0 and b"null" in _err(lib)
    assert call(w, wt, B=0) < 0 and b"empty" in _err(lib)
    assert call(w, wt, L=0) < 0 and b"empty" in _err(lib)
    assert call(w, wt, B=70000, L=2) < 0 and b"grid" in _err(lib)
    assert call(w, wt, x=P + 4) < 0 and b"aligned" in _err(lib)
    assert call(w, wt, mode=2) < 0 and b"attn_mode" in _err(lib)
    assert call(w, wt, D=1024, H=12) < 0 and b"64*H" in _err(lib)
    assert call(w, wt, F=1000) < 0 and b"multiple of 128" in _err(lib)
    assert call(w, wt, d_aw=None) < 0 and b"d_adapter_w" in _err(lib)
    assert call(_weights(False), wt, d_in=None) < 0 and b"nothing to compute" in _err(lib)
    assert call(w, _lib.BlockWeights()) < 0 and b"transposed" in _err(lib)
    # L = 1370 passes every check up to the workspace, which must hold the attention statistics as well
    need = lib.aaclip_block_backward_long_workspace_bytes(2, 1370, 1024, 4096)
    assert call(w, wt, ws_bytes=need - 1) < 0 and b"workspace" in _err(lib)
    assert call(w, wt, ws_bytes=lib.aaclip_text_backward_workspace_bytes(2 * 1370, 1024, 4096)) < 0 \
        and b"workspace" in _err(lib)
    for L in (129, 1370):
        assert call(w, wt, L=L, ws_bytes=16) < 0 and b"workspace" in _err(lib)


def test_old_entry_points_keep_their_limit():
    lib = _lib.load()
    assert lib.aaclip_attention_backward(P, P, P, 2, 129, 4, 1, 1.0, None) < 0 and b"128" in _err(lib)
    w, wt = _weights(), _weights()
    rc = lib.aaclip_block_backward(P, C.byref(w), C.byref(wt), 0.1, 2, 129, 256, 4, 1024, 1, P, P, P, P, BIG, None)
    assert rc < 0 and b"128" in _err(lib)
