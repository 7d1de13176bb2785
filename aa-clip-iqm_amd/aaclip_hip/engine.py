"""Host-side executor: turns torch tensors into raw HIP pointers and sequences
the C-ABI calls of libaaclip_hip.so.  PyTorch is used for device memory, the
current stream and parameter containers; every per-token computation is a kernel
of the library.  The torch ops that do compute are load-time weight preparation
(WeightCache: dtype conversion / transposes; FoldCache: W*gamma, its row sums and
b + W@beta, once per parameter version) -- and, outside this module, the <=16-row
anchor mean and the [B,768].[768] image score in forward_utils.py.

Layout: the residual stream is batch-first, fp32, [B*L, D] contiguous for the
whole tower (the reference permutes to LND, model/adapter.py:158; token rows are
independent so the layout is free).  Matrix-product weights are converted once to
the compute dtype and cached per parameter version.
"""
from __future__ import annotations

import collections
import ctypes as C
import os
import weakref
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import BF16, F16, F16X2, F32, BlockWeights, OverlayPlan, TilePlan

_TORCH_DT = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16, F16X2: torch.float16}
# "fp16x2": split fp16 (every matrix-product operand as an fp16 hi + lo pair, 3 MFMA products per matrix product):
# the 16-bit-MFMA mode whose taps and anomaly maps stay inside 1e-3 abs + 1e-2 rel of the fp32 reference
_PRECISION = {"fp32": F32, "f32": F32, "fp16": F16, "f16": F16, "bf16": BF16, "amp": F16, "pure_fp16": F16,
              "pure_bf16": BF16, "amp_bf16": BF16, "fp16x2": F16X2, "f16x2": F16X2, "split": F16X2}


def dtype_code(precision) -> int:
    """Map a create_model(precision=...) string (reference model/clip.py:88,
    model/model.py:63-69) to the arithmetic type of the matrix products.  The env
    var AACLIP_COMPUTE overrides it for callers that cannot pass precision."""
    env = os.environ.get("AACLIP_COMPUTE")
    if env:
        precision = env
    if isinstance(precision, int):
        return precision
    try:
        return _PRECISION[str(precision).lower()]
    except KeyError:
        raise ValueError(f"unknown precision {precision!r}; use fp32, fp16x2, fp16 or bf16")


def torch_dtype(code: int) -> torch.dtype:
    return _TORCH_DT[code]


def plain_code(code: int) -> int:
    """The arithmetic type of the side paths that have no split-fp16 GEMM kernels (IQM branch): fp32 products there.
    (Not everything on that branch is then exact fp32: with the tap levels folded, the visual cross-attention reads the
    fp16 halves of the split8 tap rows and runs p.v with fp16 probabilities, csrc/iqm.hip cross_rows_mfma_kernel.)"""
    return F32 if code == F16X2 else code


CROSS_ROWS_MAX_SEGMENTS = 4      # csrc/iqm.hip cross_rows_levels_check: tap levels one aaclip_cross_rows_levels call takes


# split fp16 (include/aaclip.h AACLIP_F16X2, csrc/common.h): fixed power-of-two scales of the e4m3 correction planes
SPLIT8_ACT_LO_EXP, SPLIT8_ACT_HI_EXP, SPLIT8_W_HI_EXP, SPLIT8_W_LO_EXP = 10, 0, 6, 17


def _e4m3_bytes(v: torch.Tensor, exp: int) -> torch.Tensor:
    """fp32 -> e4m3 (OCP e4m3fn) bytes of v * 2^exp, clamped to +-448, on v's own device (torch's conversion gives the
    same bytes on the host and on the MI355X; load-time work)."""
    x = (v.detach().float() * float(2 ** exp)).clamp_(-448.0, 448.0)
    return x.to(torch.float8_e4m3fn).view(torch.uint8)


def split16_rows(t: torch.Tensor) -> torch.Tensor:
    """fp32 [R, C] -> split16 rows [R, 2C] fp16: hi = fp16(v) | lo = fp16(v - hi) -- the attention kernel's q|k|v
    input format (what the QKV epilogue writes)."""
    v = t.detach().float()
    hi = v.to(torch.float16)
    lo = (v - hi.float()).to(torch.float16)
    return torch.cat([hi, lo], dim=-1).contiguous()


def split_rows(t: torch.Tensor, weight: bool = False, exact: bool = False) -> torch.Tensor:
    """fp32 [R, C] -> split8 rows as uint8 [R, 4C]: [hi: C x fp16][lo8: C x e4m3][hi8: C x e4m3], the GEMM operand format
    of AACLIP_F16X2 (lo8 = e4m3((v - hi) * 2^10), hi8 = e4m3(v) for activations; weights: [Wh][e4m3(W * 2^6)]
    [e4m3((W - Wh) * 2^17)], the last plane dropped when `exact`).  Load-time / caller-side operand preparation, like
    the .to(dtype) of the other modes; the hot path's own split rows are written by the kernels' epilogues."""
    v = t.detach().float()
    hi = v.to(torch.float16)
    lo = v - hi.float()
    planes = [hi.contiguous().view(torch.uint8).reshape(v.shape[0], -1)]
    if weight:
        planes.append(_e4m3_bytes(v, SPLIT8_W_HI_EXP))
        if not exact:
            planes.append(_e4m3_bytes(lo, SPLIT8_W_LO_EXP))
    else:
        planes += [_e4m3_bytes(lo, SPLIT8_ACT_LO_EXP), _e4m3_bytes(v, SPLIT8_ACT_HI_EXP)]
    return torch.cat(planes, dim=1).contiguous()


def join_split8(t: torch.Tensor, C: int) -> torch.Tensor:
    """split8 rows (uint8 [R, 4C] or fp16 [R, 2C]) -> fp64 hi + lo8 * 2^-10 (what a product sees of an activation)."""
    b = t.contiguous().view(torch.uint8).reshape(t.shape[0], -1).cpu()
    hi = b[:, : 2 * C].contiguous().view(torch.float16).double()
    lo = b[:, 2 * C: 3 * C].contiguous().view(torch.float8_e4m3fn).double() / float(2 ** SPLIT8_ACT_LO_EXP)
    return hi + lo


BACKWARD_PRECISIONS = ("fp32", "bf16x3")   # arithmetic of the visual blocks' backward (autograd.backward_precision)


def backward_precision_name(precision) -> str:
    name = str(precision).lower()
    if name not in BACKWARD_PRECISIONS:
        raise ValueError(f"unknown backward precision {precision!r}; use fp32 or bf16x3")
    return name


def split3_weight(w: torch.Tensor, q_rows: int = 0) -> torch.Tensor:
    """[N, K] -> the stacked bf16 weight [N, 3K] = [Wh | Wh | Wl] of the bf16x3 backward (include/aaclip.h): Wh =
    bf16(w), Wl = bf16(w - Wh).  Against split3 rows [Ah | Al | Ah] a plain bf16 product over 3K sums Ah.Wh + Al.Wh +
    Ah.Wl.  q_rows: that many leading rows are multiplied by 1/8 first (the q scale, a power of two: exact).  Pure
    torch, on w's device; load-time work (WeightCache)."""
    v = w.detach().float()
    if q_rows:
        v = v.clone()
        v[:q_rows] *= 0.125
    hi = v.to(torch.bfloat16)
    lo = (v - hi.float()).to(torch.bfloat16)
    return torch.cat([hi, hi, lo], dim=1).contiguous()


def split3_rows(x: torch.Tensor) -> torch.Tensor:
    """fp32 [rows, K] -> split3 rows, bf16 [rows, 3K] = [hi | lo | hi] (aaclip_split3_rows); K a multiple of 64."""
    require_gpu(x, "split3_rows")
    x = _f32c(x)
    rows, K = x.shape
    out = torch.empty(rows, 3 * K, dtype=torch.bfloat16, device=x.device)
    _lib.check(_lib.load().aaclip_split3_rows(x.data_ptr(), out.data_ptr(), rows, K, _stream(x.device)), "split3_rows")
    return out


def _stream(dev: torch.device) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def require_gpu(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(
            f"{what}: tensor is on {t.device}; the AA-CLIP HIP path only runs on an MI355X (cuda) device "
            "and has no CPU fallback")


class Workspace:
    """One growing scratch buffer per device (caller-owned as far as the C ABI
    is concerned)."""
    _bufs: Dict[tuple, torch.Tensor] = {}

    @classmethod
    def get(cls, dev: torch.device, nbytes: int) -> torch.Tensor:
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        idx = (idx, torch.cuda.current_stream(dev).cuda_stream)   # one scratch buffer per (device, stream)
        buf = cls._bufs.get(idx)
        if buf is None or buf.numel() < nbytes:
            cls._bufs[idx] = None
            buf = torch.empty(int(nbytes * 1.02) + 4096, dtype=torch.uint8, device=dev)
            cls._bufs[idx] = buf
        return buf

    @classmethod
    def for_rows(cls, dev: torch.device, code: int, rows: int, D: int, F: int, E: int) -> torch.Tensor:
        n = _lib.load().aaclip_workspace_bytes(code, rows, D, F, E)
        return cls.get(dev, n)


def _f32c(t: torch.Tensor) -> torch.Tensor:
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


class WeightCache:
    """Converted copies of matrix weights, one per (parameter object, dtype, kind),
    refreshed when the parameter's storage or version changes (adapters are
    trainable).  Entries hold a weak reference to the parameter: id() values and
    device addresses are recycled once a model is freed, so identity is checked
    on the object itself and dead entries are dropped."""

    def __init__(self):
        self._c: Dict[Tuple[int, int, str], tuple] = {}

    def get(self, p: torch.Tensor, code: int, kind: str = "plain") -> torch.Tensor:
        """kind: 'plain' | 'transpose' | 'conv', or one of the bf16x3 backward's (code BF16: 'split3' the stacked weight
        of split3_weight, 'split3_t' the same of the transpose, 'split3_q' the stacked in_proj weight with its q rows
        times 1/8; code F32: 'scale_q' the in_proj bias with its q entries times 1/8).
        Code F16X2: split8 weight rows as uint8 [out, 4*in]; with a '+exact'
        suffix the 3-plane form [out, 3*in] when every value is exact in fp16 and in_features is a multiple of 256
        (the kernels then skip the weight-lo correction tile) -- tell them apart by the shape."""
        key = (id(p), code, kind)
        hit = self._c.get(key)
        if hit is not None and hit[0]() is p and hit[1] == p.data_ptr() and hit[2] == p._version:
            return hit[3]
        src = p.detach()
        allow_exact = kind.endswith("+exact")
        kind = kind.split("+")[0]
        if kind in ("split3", "split3_t", "split3_q"):
            out = split3_weight(src.t() if kind == "split3_t" else src,
                                q_rows=src.shape[0] // 3 if kind == "split3_q" else 0)
            return self._put(key, p, out)
        if kind == "scale_q":
            out = src.float().clone()
            out[: out.shape[0] // 3] *= 0.125
            return self._put(key, p, out)
        if kind == "transpose":          # [in, out] parameter used as x @ P  ->  [out, in]
            src = src.t()
        elif kind == "conv":             # conv1.weight [D,3,ps,ps] -> [D, Kpad]
            d = src.shape[0]
            flat = src.reshape(d, -1)
            kpad = (flat.shape[1] + 63) // 64 * 64
            pad = torch.zeros(d, kpad, dtype=flat.dtype, device=flat.device)
            pad[:, : flat.shape[1]] = flat
            src = pad
        if code == F16X2:
            src32 = src.float()
            exact = (allow_exact and src.shape[1] % 256 == 0
                     and bool((src32.to(torch.float16).float() == src32).all()))
            out = split_rows(src32, weight=True, exact=exact)
        else:
            out = src.to(_TORCH_DT[code]).contiguous()
        return self._put(key, p, out)

    def _put(self, key, p: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        cache = self._c

        def _drop(_ref, key=key):
            ent = cache.get(key)
            if ent is not None and ent[0] is _ref:
                del cache[key]

        self._c[key] = (weakref.ref(p, _drop), p.data_ptr(), p._version, out)
        return out


CACHE = WeightCache()


class FoldCache:
    """ln_2 folded into c_fc (include/aaclip.h, aaclip_block_weights): per block and dtype
    (c_fc.weight * ln_2.weight in the compute dtype, its row sums, c_fc.bias + c_fc.weight @ ln_2.bias),
    rebuilt when any of the four parameters changes."""

    def __init__(self):
        self._c: Dict[Tuple[int, int], tuple] = {}

    @staticmethod
    def _fold(weight, bias, gamma, beta, code):
        fw, fb, g, be = (p.detach().float() for p in (weight, bias, gamma, beta))
        wf = (fw * g[None, :]).to(_TORCH_DT[code]).contiguous()
        return wf, wf.float().sum(dim=1).contiguous(), (fb + fw @ be).contiguous()

    def get(self, block, code: int):
        """-> (fc_w_fold, fc_fold_s, fc_fold_b, qkv_w_fold, qkv_fold_s, qkv_fold_b)"""
        ps = (block.mlp.c_fc.weight, block.mlp.c_fc.bias, block.ln_2.weight, block.ln_2.bias,
              block.attn.in_proj_weight, block.attn.in_proj_bias, block.ln_1.weight, block.ln_1.bias)
        sig = tuple((p.data_ptr(), p._version) for p in ps)
        key = (id(block), code)
        hit = self._c.get(key)
        if hit is not None and hit[0]() is block and hit[1] == sig:
            return hit[2]
        with torch.no_grad():
            out = self._fold(*ps[:4], code) + self._fold(*ps[4:], code)
        cache = self._c

        def _drop(_ref, key=key):
            ent = cache.get(key)
            if ent is not None and ent[0] is _ref:
                del cache[key]

        self._c[key] = (weakref.ref(block, _drop), sig, out)
        return out


FOLDS = FoldCache()


def _keep(refs: list, t: torch.Tensor) -> int:
    refs.append(t)
    return t.data_ptr()


def pack_block(block, code: int, adapter_weight: Optional[torch.Tensor]) -> Tuple[BlockWeights, list]:
    """Build the aaclip_block_weights struct for one ResidualAttentionBlock module."""
    refs: list = []
    w = BlockWeights()
    w.ln1_w = _keep(refs, _f32c(block.ln_1.weight))
    w.ln1_b = _keep(refs, _f32c(block.ln_1.bias))
    ex = 0

    def mat(param, bit):
        """matrix weight in the compute dtype; split fp16: plain fp16 + its exact16 bit when the lo half is zero"""
        nonlocal ex
        if code != F16X2:
            return _keep(refs, CACHE.get(param, code))
        t = CACHE.get(param, code, "plain+exact")
        if t.shape[1] == 3 * param.shape[1]:
            ex |= bit
        return _keep(refs, t)

    w.qkv_w = mat(block.attn.in_proj_weight, _lib.EXACT16_QKV)
    w.qkv_b = _keep(refs, _f32c(block.attn.in_proj_bias))
    w.out_w = mat(block.attn.out_proj.weight, _lib.EXACT16_OUT)
    w.out_b = _keep(refs, _f32c(block.attn.out_proj.bias))
    w.ln2_w = _keep(refs, _f32c(block.ln_2.weight))
    w.ln2_b = _keep(refs, _f32c(block.ln_2.bias))
    w.fc_w = mat(block.mlp.c_fc.weight, _lib.EXACT16_FC)
    w.fc_b = _keep(refs, _f32c(block.mlp.c_fc.bias))
    w.proj_w = mat(block.mlp.c_proj.weight, _lib.EXACT16_PROJ)
    w.proj_b = _keep(refs, _f32c(block.mlp.c_proj.bias))
    w.adapter_w = mat(adapter_weight, _lib.EXACT16_ADAPTER) if adapter_weight is not None else None
    w.exact16 = ex
    if code in (F16, BF16):
        wf, fs, fb, qf, qs, qb = FOLDS.get(block, code)
        w.fc_w_fold, w.fc_fold_s, w.fc_fold_b = _keep(refs, wf), _keep(refs, fs), _keep(refs, fb)
        w.qkv_w_fold, w.qkv_fold_s, w.qkv_fold_b = _keep(refs, qf), _keep(refs, qs), _keep(refs, qb)
    return w, refs


# ----------------------------------------------------------------------------
# path-level calls
# ----------------------------------------------------------------------------
def patch_embed(img: torch.Tensor, visual, code: int) -> Tuple[torch.Tensor, int, int]:
    """reference model/adapter.py:139-156 -> x [B*L, D] fp32, returns (x, B, L)."""
    require_gpu(img, "patch_embed")
    lib = _lib.load()
    img = _f32c(img)
    B, Cc, H, W = img.shape
    if Cc != 3:
        raise ValueError("patch_embed expects [B,3,H,W] images")
    ps = visual.patch_size[0]
    D = visual.embed_dim
    L = (H // ps) * (W // ps) + 1
    pos = _f32c(visual.positional_embedding)
    if pos.shape[0] != L:
        raise RuntimeError(f"positional_embedding has {pos.shape[0]} rows but the image needs {L}")
    x = torch.empty(B * L, D, dtype=torch.float32, device=img.device)
    ws = Workspace.for_rows(img.device, code, B * L, D, 4 * D, 0)
    conv_w = CACHE.get(visual.conv1.weight, code, "conv")
    cls, lw, lb = _f32c(visual.class_embedding), _f32c(visual.ln_pre.weight), _f32c(visual.ln_pre.bias)
    _lib.check(lib.aaclip_patch_embed(img.data_ptr(), conv_w.data_ptr(), cls.data_ptr(), pos.data_ptr(),
                                      lw.data_ptr(), lb.data_ptr(), x.data_ptr(), B, H, W, ps, D, code,
                                      ws.data_ptr(), ws.numel(), _stream(img.device)), "patch_embed")
    return x, B, L


ATTN_FULL, ATTN_CAUSAL, ATTN_VV_BATCH = 0, 1, 2


def run_block(x: torch.Tensor, block, B: int, L: int, heads: int, code: int, causal: bool = False,
              adapter_weight: Optional[torch.Tensor] = None, mix: float = 0.0) -> None:
    """In place on x [B*L, D]: reference model/transformer.py:239-258 (+ adapter.py:163-170).
    A block flagged by VisionTransformer.DAPM_replace (`block.surgery`) runs the V-V attention over
    the batch axis (reference transformer.py:102-152 as executed, include/aaclip.h AACLIP_ATTN_VV_BATCH)."""
    run_blocks(x, [block], B, L, heads, code, causal=causal, adapter_weights=[adapter_weight], mix=mix)


def run_blocks(x: torch.Tensor, blocks: Sequence, B: int, L: int, heads: int, code: int, causal: bool = False,
               adapter_weights: Optional[Sequence[Optional[torch.Tensor]]] = None, mix: float = 0.0,
               x_out: Optional[torch.Tensor] = None, x_outs: Optional[Sequence[torch.Tensor]] = None) -> None:
    """Consecutive blocks in ONE aaclip_blocks call (in place on x [B*L, D]); nothing reads x in between, so
    the library folds ln_1 of every block but the first into its QKV product.  Blocks flagged by
    DAPM_replace run their V-V attention; a run must not mix the two attention modes.
    x_out: leave x untouched and continue the stream in x_out (aaclip_blocks_to) -- x stays valid as a tap.
    x_outs: one tensor per block = the buffer holding the stream after that block (aaclip_blocks_taps): a buffer
    that later blocks do not write again is a tap, and the whole tower is one call."""
    blocks = list(blocks)
    if not blocks:
        return
    if len({bool(getattr(b, "surgery", False)) for b in blocks}) > 1:
        raise ValueError("run_blocks: split the run where the attention mode changes")
    mode = int(causal)
    if getattr(blocks[0], "surgery", False):
        if causal:
            raise ValueError("the V-V attention block takes no mask")
        mode = ATTN_VV_BATCH
    require_gpu(x, "block")
    lib = _lib.load()
    D = x.shape[1]
    F = blocks[0].mlp.c_fc.weight.shape[0]
    arr = (BlockWeights * len(blocks))()
    refs = []
    for i, blk in enumerate(blocks):
        aw = adapter_weights[i] if adapter_weights is not None else None
        w, r = pack_block(blk, code, aw)
        arr[i] = w
        refs.append(r)
    ws = Workspace.for_rows(x.device, code, B * L, D, F, 0)
    if x_out is not None:
        require_gpu(x_out, "block")
        if x_out.shape != x.shape or x_out.dtype != torch.float32 or not x_out.is_contiguous():
            raise ValueError("x_out must be a contiguous fp32 tensor of x's shape")
    if x_outs is not None:
        if x_out is not None or len(x_outs) != len(blocks):
            raise ValueError("x_outs: one output tensor per block (and no x_out)")
        ptrs = (C.c_void_p * len(blocks))()
        for i, t in enumerate(x_outs):
            require_gpu(t, "block")
            if t.shape != x.shape or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("x_outs must be contiguous fp32 tensors of x's shape")
            ptrs[i] = t.data_ptr()
        _lib.check(lib.aaclip_blocks_taps(x.data_ptr(), ptrs, arr, len(blocks), float(mix), B, L, D, heads, F, mode,
                                          code, ws.data_ptr(), ws.numel(), _stream(x.device)), "blocks")
        del refs
        return
    dst = x if x_out is None else x_out
    _lib.check(lib.aaclip_blocks_to(x.data_ptr(), dst.data_ptr(), arr, len(blocks), float(mix), B, L, D, heads, F, mode,
                                    code, ws.data_ptr(), ws.numel(), _stream(x.device)), "blocks")
    del refs


def tap_head(x: torch.Tensor, ln_post, proj_weight: torch.Tensor, act: bool, B: int, L: int, code: int,
             det_weight: Optional[torch.Tensor] = None, keep_rows: bool = False):
    """reference model/adapter.py:171-184 -> (seg [B,L-1,E] unit rows, det [B,E] or None).
    keep_rows: also return ln_post(x) [B*L, .] in the layout of `code` (uint8 [B*L, 4D] split8 rows under fp16x2): the
    IQM branch reads the same rows (reference model/adapter.py:205-208)."""
    require_gpu(x, "tap_head")
    lib = _lib.load()
    D, E = x.shape[1], proj_weight.shape[0]
    seg = torch.empty(B, L - 1, E, dtype=torch.float32, device=x.device)
    det = torch.empty(B, E, dtype=torch.float32, device=x.device) if det_weight is not None else None
    pw = CACHE.get(proj_weight, code)
    dw = CACHE.get(det_weight, code) if det_weight is not None else None
    lw, lb = _f32c(ln_post.weight), _f32c(ln_post.bias)
    ws = Workspace.for_rows(x.device, code, B * L, D, 0, E)
    if keep_rows:
        rows = (torch.empty(B * L, 4 * D, dtype=torch.uint8, device=x.device) if code == F16X2
                else torch.empty(B * L, D, dtype=torch_dtype(code), device=x.device))
        _lib.check(lib.aaclip_tap_head_keep_rows(x.data_ptr(), lw.data_ptr(), lb.data_ptr(), pw.data_ptr(), int(act),
                                                 seg.data_ptr(), _ptr(dw), _ptr(det), rows.data_ptr(), B, L, D, E, code,
                                                 ws.data_ptr(), ws.numel(), _stream(x.device)), "tap_head_keep_rows")
        return seg, det, rows
    _lib.check(lib.aaclip_tap_head(x.data_ptr(), lw.data_ptr(), lb.data_ptr(), pw.data_ptr(), int(act),
                                   seg.data_ptr(), _ptr(dw), _ptr(det), B, L, D, E, code, ws.data_ptr(), ws.numel(),
                                   _stream(x.device)), "tap_head")
    return seg, det


def row_head(x: torch.Tensor, tokens: Optional[torch.Tensor], ln, proj: torch.Tensor, kind: str, act: bool, n: int,
             T: int, mode: int, code: int) -> torch.Tensor:
    """LayerNorm + row pick + projection (reference model/adapter.py:297-299,
    model/model.py:198-200, model/transformer.py:542-546).  kind: 'plain' for an
    [E,D] Linear weight, 'transpose' for a [D,E] projection parameter."""
    require_gpu(x, "row_head")
    lib = _lib.load()
    D = x.shape[1]
    pw = CACHE.get(proj, code, kind)
    E = pw.shape[0]
    out = torch.empty(n, E, dtype=torch.float32, device=x.device)
    lw, lb = _f32c(ln.weight), _f32c(ln.bias)
    ws = Workspace.for_rows(x.device, code, n * T + n, D, 0, E)
    tk = None
    if tokens is not None:
        tk = tokens.to(device=x.device, dtype=torch.int32).contiguous()
    _lib.check(lib.aaclip_row_head(x.data_ptr(), _ptr(tk), lw.data_ptr(), lb.data_ptr(), pw.data_ptr(), int(act),
                                   out.data_ptr(), n, T, D, E, mode, code, ws.data_ptr(), ws.numel(),
                                   _stream(x.device)), "row_head")
    return out


def text_embed(tokens: torch.Tensor, table: torch.Tensor, pos: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """reference model/adapter.py:277-281 -> (x [n*T, D] fp32, int32 tokens on device)."""
    lib = _lib.load()
    table = _f32c(table)
    require_gpu(table, "text_embed")
    tk = tokens.to(device=table.device, dtype=torch.int32).contiguous()
    n, T = tk.shape
    pos = _f32c(pos)
    if pos.shape[0] < T:
        raise RuntimeError("text longer than the positional embedding")
    D = table.shape[1]
    x = torch.empty(n * T, D, dtype=torch.float32, device=table.device)
    _lib.check(lib.aaclip_text_embed(tk.data_ptr(), table.data_ptr(), pos.data_ptr(), x.data_ptr(), n, T, D,
                                     table.shape[0], _stream(table.device)), "text_embed")
    return x, tk


def layernorm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-5,
              out_code: int = F32) -> torch.Tensor:
    """reference model/transformer.py:37-43 on any [..., D] tensor."""
    require_gpu(x, "layernorm")
    lib = _lib.load()
    xc = _f32c(x)
    D = xc.shape[-1]
    rows = xc.numel() // D
    oshape = xc.shape if out_code != F16X2 else (*xc.shape[:-1], 2 * D)   # split8 rows: 4 bytes per element
    out = torch.empty(oshape, dtype=_TORCH_DT[out_code], device=x.device)
    w, b = _f32c(weight), _f32c(bias)
    _lib.check(lib.aaclip_layernorm(xc.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), out_code, rows, D,
                                    float(eps), _stream(x.device)), "layernorm")
    return out


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], act: bool, code: int,
           kind: str = "plain") -> torch.Tensor:
    """y = act(x W^T [+ b]) through the HIP GEMM (used by SimpleAdapter/SimpleProj
    when a caller invokes those modules directly)."""
    require_gpu(x, "linear")
    lib = _lib.load()
    K = x.shape[-1]
    w = CACHE.get(weight, code, kind)
    N = w.shape[0]
    a = x.detach().reshape(-1, K)
    a = split_rows(a) if code == F16X2 else a.to(_TORCH_DT[code]).contiguous()
    out = torch.empty(a.shape[0], N, dtype=torch.float32, device=x.device)
    b = _f32c(bias) if bias is not None else None
    lda = 2 * K if code == F16X2 else K            # split8 rows: 4 bytes per element = 2K halves
    _lib.check(lib.aaclip_gemm(code, _lib.EPI_ACT_F32, a.data_ptr(), lda, w.data_ptr(), _ptr(b), out.data_ptr(), N,
                               a.shape[0], N, K, int(act), 0, 1.0, _stream(x.device)), "gemm")
    return out.reshape(*x.shape[:-1], N)


def anomaly_map(seg_tokens: Sequence[torch.Tensor], text_feature: torch.Tensor, img_size: int, ksize: int,
                sigma: float) -> torch.Tensor:
    """Fused reference forward_utils.py:196-213 (test=True) over all levels + the
    level sum of test_last.py:95-100,149 -> [B, S, S]."""
    lib = _lib.load()
    segs = [_f32c(s) for s in seg_tokens]
    require_gpu(segs[0], "anomaly_map")
    B, P, E = segs[0].shape
    g = int(round(P ** 0.5))
    if g * g != P:
        raise ValueError(f"{P} patches is not a square grid")
    tf = _f32c(text_feature).to(segs[0].device)
    if tf.dim() == 2:
        stride = 0
    elif tf.dim() == 3 and tf.shape[0] == B:
        stride = E * 2
    else:
        raise ValueError("text feature must be [E,2] or [B,E,2]")
    if tf.shape[-1] != 2 or tf.shape[-2] != E:
        raise ValueError("text feature must have shape [..., E, 2]")
    out = torch.empty(B, img_size, img_size, dtype=torch.float32, device=segs[0].device)
    ws = Workspace.get(segs[0].device, len(segs) * B * P * 4 + 256)
    arr = (C.c_void_p * len(segs))(*[s.data_ptr() for s in segs])
    _lib.check(lib.aaclip_anomaly_map(arr, len(segs), tf.data_ptr(), stride, out.data_ptr(), B, g, E, img_size,
                                      ksize, float(sigma), ws.data_ptr(), ws.numel(), _stream(out.device)),
               "anomaly_map")
    return out


def similarity_map_train(seg: torch.Tensor, text_feature: torch.Tensor, img_size: int) -> torch.Tensor:
    """reference forward_utils.py:196-216 with test=False -> [B, 2, S, S]."""
    lib = _lib.load()
    seg = _f32c(seg)
    require_gpu(seg, "similarity_map")
    B, P, E = seg.shape
    g = int(round(P ** 0.5))
    if g * g != P:
        raise ValueError(f"{P} patches is not a square grid")
    tf = _f32c(text_feature).to(seg.device)
    stride = 0 if tf.dim() == 2 else E * 2
    if tf.shape[-1] != 2:
        raise AssertionError("C == 2 expected")
    out = torch.empty(B, 2, img_size, img_size, dtype=torch.float32, device=seg.device)
    ws = Workspace.get(seg.device, 2 * B * P * 4 + 256)
    _lib.check(lib.aaclip_similarity_map_train(seg.data_ptr(), tf.data_ptr(), stride, out.data_ptr(), B, g, E,
                                               img_size, ws.data_ptr(), ws.numel(), _stream(out.device)),
               "similarity_map_train")
    return out


def similarity_map_train_backward(seg: torch.Tensor, text_feature: torch.Tensor, preds: torch.Tensor,
                                  d_preds: torch.Tensor, need_seg: bool = False, need_anchors: bool = True):
    """Backward of similarity_map_train: (d seg [B,P,E] or None, d text_feature (its shape) or None)."""
    lib = _lib.load()
    seg = _f32c(seg)
    require_gpu(seg, "similarity_map_train_backward")
    B, P, E = seg.shape
    g = int(round(P ** 0.5))
    tf = _f32c(text_feature).to(seg.device)
    if tf.shape not in ((E, 2), (B, E, 2)):
        raise ValueError(f"text feature must be [{E}, 2] or [{B}, {E}, 2], got {tuple(tf.shape)}")
    stride = 0 if tf.dim() == 2 else E * 2
    S = preds.shape[-1]
    preds, d_preds = _f32c(preds), _f32c(d_preds)
    if preds.shape != (B, 2, S, S) or d_preds.shape != preds.shape:
        raise ValueError("preds / d_preds must be [B, 2, S, S]")
    d_seg = torch.empty_like(seg) if need_seg else None
    d_tf = torch.empty_like(tf) if need_anchors else None
    ws = Workspace.get(seg.device, lib.aaclip_similarity_map_train_backward_workspace_bytes(B, g, S))
    _lib.check(lib.aaclip_similarity_map_train_backward(seg.data_ptr(), tf.data_ptr(), stride, preds.data_ptr(),
                                                        d_preds.data_ptr(), _ptr(d_tf), _ptr(d_seg), B, g, E, S,
                                                        ws.data_ptr(), ws.numel(), _stream(seg.device)),
               "similarity_map_train_backward")
    return d_seg, d_tf


def _iqm_train_shapes(seg: torch.Tensor, queries: torch.Tensor, what: str):
    require_gpu(seg, what)
    B, P, E = seg.shape
    g = int(round(P ** 0.5))
    if g * g != P:
        raise AssertionError(f"L={P} is not a perfect square")         # reference train.py:196
    if queries.shape != (B, 2, E):
        raise ValueError(f"{what}: queries must be [{B}, 2, {E}] (normal, abnormal), got {tuple(queries.shape)}")
    return B, P, E, g


def iqm_map_train(seg: torch.Tensor, queries: torch.Tensor, img_size: int):
    """reference train.py:173-209, one tap level -> (out [B, 2, S, S] = the half-pixel bilinear upsample of (1 - p, p),
    grid [B, P] = p = sigmoid(cos(f, q_abnormal) - cos(f, q_normal)), which the backward reads)."""
    lib = _lib.load()
    seg = _f32c(seg)
    B, P, E, g = _iqm_train_shapes(seg, queries, "iqm_map_train")
    q = _f32c(queries).to(seg.device)
    S = int(img_size)
    out = torch.empty(B, 2, S, S, dtype=torch.float32, device=seg.device)
    grid = torch.empty(B, P, dtype=torch.float32, device=seg.device)
    _lib.check(lib.aaclip_iqm_map_train(seg.data_ptr(), q.data_ptr(), grid.data_ptr(), out.data_ptr(), B, g, E, S,
                                        _stream(seg.device)), "iqm_map_train")
    return out, grid


def iqm_map_train_backward(seg: torch.Tensor, queries: torch.Tensor, grid: torch.Tensor, d_preds: torch.Tensor,
                           need_seg: bool = True, need_queries: bool = True):
    """Backward of iqm_map_train: (d seg [B, P, E] or None, d queries [B, 2, E] or None)."""
    lib = _lib.load()
    seg = _f32c(seg)
    B, P, E, g = _iqm_train_shapes(seg, queries, "iqm_map_train_backward")
    if not (need_seg or need_queries):
        raise ValueError("iqm_map_train_backward: nothing to compute")
    q, grid, d_preds = _f32c(queries).to(seg.device), _f32c(grid), _f32c(d_preds)
    S = d_preds.shape[-1]
    if d_preds.shape != (B, 2, S, S) or grid.shape != (B, P):
        raise ValueError("iqm_map_train_backward: d_preds must be [B, 2, S, S] and grid [B, P]")
    d_seg = torch.empty_like(seg) if need_seg else None
    d_q = torch.empty_like(q) if need_queries else None
    ws = Workspace.get(seg.device, lib.aaclip_iqm_map_train_backward_workspace_bytes(B, g, E, S))
    _lib.check(lib.aaclip_iqm_map_train_backward(seg.data_ptr(), q.data_ptr(), grid.data_ptr(), d_preds.data_ptr(),
                                                 _ptr(d_seg), _ptr(d_q), B, g, E, S, ws.data_ptr(), ws.numel(),
                                                 _stream(seg.device)), "iqm_map_train_backward")
    return d_seg, d_q


def _seg_loss_layout(preds: torch.Tensor, mask: torch.Tensor):
    """preds [B,2,S,S] (or [B,S,S] / [B,P] for a single channel) + mask with B*P elements -> (B, P, img_stride,
    chan_stride, fp32 contiguous mask)."""
    if preds.dim() == 4:
        if preds.shape[1] != 2:
            raise ValueError("seg loss: preds must have 2 channels")
        B, P = preds.shape[0], preds.shape[2] * preds.shape[3]
        istr, cstr = 2 * P, P
    else:
        B, P = preds.shape[0], preds[0].numel()
        istr, cstr = P, 0
    m = _f32c(mask).to(preds.device)
    if m.numel() != B * P:
        raise ValueError(f"seg loss: mask has {m.numel()} elements, preds need {B * P} (one value per pixel)")
    return B, P, istr, cstr, m


def seg_loss(preds: torch.Tensor, mask: torch.Tensor, terms: int = _lib.SEG_LOSS_ALL):
    """reference forward_utils.py:223-227 (and its FocalLoss / BinaryDiceLoss) -> (loss [4] = {total, focal, dice0,
    dice1}, coef [B,4] for seg_loss_backward)."""
    lib = _lib.load()
    preds = _f32c(preds)
    require_gpu(preds, "seg_loss")
    B, P, istr, cstr, m = _seg_loss_layout(preds, mask)
    loss = torch.empty(4, dtype=torch.float32, device=preds.device)
    coef = torch.empty(B, 4, dtype=torch.float32, device=preds.device)
    ws = Workspace.get(preds.device, lib.aaclip_seg_loss_workspace_bytes(B))
    _lib.check(lib.aaclip_seg_loss(preds.data_ptr(), istr, cstr, m.data_ptr(), int(terms), loss.data_ptr(),
                                   coef.data_ptr(), B, P, ws.data_ptr(), ws.numel(), _stream(preds.device)), "seg_loss")
    return loss, coef


def seg_loss_backward(preds: torch.Tensor, mask: torch.Tensor, coef: torch.Tensor, d_loss: torch.Tensor,
                      terms: int = _lib.SEG_LOSS_ALL) -> torch.Tensor:
    """d preds (preds' shape; zeros in a channel no term reads) from d loss [4]."""
    lib = _lib.load()
    preds = _f32c(preds)
    require_gpu(preds, "seg_loss_backward")
    B, P, istr, cstr, m = _seg_loss_layout(preds, mask)
    d = torch.zeros_like(preds) if terms != _lib.SEG_LOSS_ALL else torch.empty_like(preds)
    dl = _f32c(d_loss).to(preds.device).reshape(4)
    _lib.check(lib.aaclip_seg_loss_backward(preds.data_ptr(), istr, cstr, m.data_ptr(), int(terms), coef.data_ptr(),
                                            dl.data_ptr(), d.data_ptr(), B, P, _stream(preds.device)),
               "seg_loss_backward")
    return d


# ------------------------------------------------------------------------------------------------
# backward of the adapted text tower (include/aaclip.h, "backward of the adapted text tower"): fp32, thin wrappers
def text_backward_workspace(dev: torch.device, rows: int, D: int, F: int) -> torch.Tensor:
    return Workspace.get(dev, _lib.load().aaclip_text_backward_workspace_bytes(int(rows), int(D), int(F)))


def gemm_wgrad(dz: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """dw[o, i] = sum_r dz[r, o] u[r, i] for fp32 dz [rows, O], u [rows, I] -> fp32 [O, I] (aaclip_gemm_wgrad)."""
    require_gpu(dz, "gemm_wgrad")
    dz, u = _f32c(dz), _f32c(u)
    rows, O = dz.shape
    I = u.shape[1]
    dw = torch.empty(O, I, dtype=torch.float32, device=dz.device)
    ws = text_backward_workspace(dz.device, rows, I, 0)
    _lib.check(_lib.load().aaclip_gemm_wgrad(dz.data_ptr(), O, u.data_ptr(), I, dw.data_ptr(), rows, O, I, ws.data_ptr(),
                                             ws.numel(), _stream(dz.device)), "gemm_wgrad")
    return dw


ATTN_BWD_SHORT_MAX_L = 128   # csrc/kernels.h ATTN_BWD_MAX_L: the longest row of aaclip_attention_backward


def _long_rows(L: int, long_rows: Optional[bool]) -> bool:
    """Which backward entry serves rows of length L: None = the short one up to 128 tokens (unchanged bits for the text
    tower), the tiled *_long one above; True forces the tiled kernels at any L."""
    return L > ATTN_BWD_SHORT_MAX_L if long_rows is None else bool(long_rows)


def _backward_route(L: int, long_rows: Optional[bool], precision: str) -> str:
    """The key of _ATTN_BWD / _BLOCK_BWD: "bf16x3" at any L, else "long" or "short" by _long_rows."""
    return "bf16x3" if precision == "bf16x3" else "long" if _long_rows(L, long_rows) else "short"


_ATTN_BWD = {   # route -> (entry, its workspace-size function or None, error tag)
    "short": ("aaclip_attention_backward", None, "attention_backward"),
    "long": ("aaclip_attention_backward_long", "aaclip_attention_backward_long_workspace_bytes", "attention_backward_long"),
    "bf16x3": ("aaclip_attention_backward_long_bf16x3", "aaclip_attention_backward_long_bf16x3_workspace_bytes",
               "attention_backward_long_bf16x3"),
}


def attention_backward(qkv: torch.Tensor, d_ctx: torch.Tensor, B: int, L: int, heads: int, causal: bool,
                       dq_scale: float = 1.0, long_rows: Optional[bool] = None, precision: str = "fp32") -> torch.Tensor:
    """packed fp32 q|k|v rows [B*L, 3*H*64] (q pre-scaled) + d ctx [B*L, H*64] -> d qkv: aaclip_attention_backward for
    L <= 128, aaclip_attention_backward_long above (long_rows: see _long_rows).  precision "bf16x3": the tiled
    three-term bf16 entry (aaclip_attention_backward_long_bf16x3) at any L."""
    precision = backward_precision_name(precision)
    require_gpu(qkv, "attention_backward")
    qkv, d_ctx = _f32c(qkv), _f32c(d_ctx)
    out = torch.empty_like(qkv)
    lib = _lib.load()
    entry, ws_bytes, tag = _ATTN_BWD[_backward_route(L, long_rows, precision)]
    ws_args = ()
    if ws_bytes is not None:
        ws = Workspace.get(qkv.device, getattr(lib, ws_bytes)(int(B), int(L), int(heads)))
        ws_args = (ws.data_ptr(), ws.numel())
    _lib.check(getattr(lib, entry)(qkv.data_ptr(), d_ctx.data_ptr(), out.data_ptr(), B, L, heads, int(causal),
                                   float(dq_scale), *ws_args, _stream(qkv.device)), tag)
    return out


def layernorm_backward(x: torch.Tensor, weight: torch.Tensor, d_y: torch.Tensor, d_resid: Optional[torch.Tensor] = None,
                       eps: float = 1e-5) -> torch.Tensor:
    """LayerNorm input gradient of fp32 rows [rows, D] (+ d_resid)."""
    require_gpu(x, "layernorm_backward")
    x, d_y, w = _f32c(x), _f32c(d_y), _f32c(weight)
    r = _f32c(d_resid) if d_resid is not None else None
    D = x.shape[-1]
    out = torch.empty_like(x)
    _lib.check(_lib.load().aaclip_layernorm_backward(x.data_ptr(), w.data_ptr(), d_y.data_ptr(), _ptr(r), out.data_ptr(),
                                                     x.numel() // D, D, float(eps), _stream(x.device)),
               "layernorm_backward")
    return out


def adapter_mix_backward(u: torch.Tensor, z: torch.Tensor, d_y: torch.Tensor, weight: float):
    """-> (d z, direct d u) of y = weight * a |u| / |a| + (1 - weight) * u, a = LeakyReLU(z); fp32 rows [rows, D]."""
    require_gpu(u, "adapter_mix_backward")
    u, z, d_y = _f32c(u), _f32c(z), _f32c(d_y)
    D = u.shape[-1]
    d_z, d_u = torch.empty_like(u), torch.empty_like(u)
    _lib.check(_lib.load().aaclip_adapter_mix_backward(u.data_ptr(), z.data_ptr(), d_y.data_ptr(), d_z.data_ptr(),
                                                       d_u.data_ptr(), u.numel() // D, D, float(weight),
                                                       _stream(u.device)), "adapter_mix_backward")
    return d_z, d_u


# The weight structs of the block backward beside pack_block's: per field the (dtype code, WeightCache kind) of its copy
_MATRICES = ("qkv_w", "out_w", "fc_w", "proj_w")
_BLOCK_PACKS = {
    "transposed": {f: (F32, "transpose") for f in _MATRICES + ("adapter_w",)},
    "split3": dict({f: (BF16, "split3") for f in _MATRICES}, qkv_w=(BF16, "split3_q"), qkv_b=(F32, "scale_q")),
    "split3_transposed": dict({f: (BF16, "split3_t") for f in _MATRICES}, adapter_w=(F32, "transpose")),
}


def _pack_block_copies(block, adapter_weight: Optional[torch.Tensor], pack: str) -> Tuple[BlockWeights, list]:
    params = dict(qkv_w=block.attn.in_proj_weight, qkv_b=block.attn.in_proj_bias, out_w=block.attn.out_proj.weight,
                  fc_w=block.mlp.c_fc.weight, proj_w=block.mlp.c_proj.weight, adapter_w=adapter_weight)
    refs: list = []
    w = BlockWeights()
    for field, (code, kind) in _BLOCK_PACKS[pack].items():
        if field != "adapter_w" or adapter_weight is not None:
            setattr(w, field, _keep(refs, CACHE.get(params[field], code, kind)))
    return w, refs


def pack_block_transposed(block, adapter_weight: Optional[torch.Tensor]) -> Tuple[BlockWeights, list]:
    """The `wt` argument of aaclip_block_backward: fp32 transposes [in, out] of the block's matrix weights."""
    return _pack_block_copies(block, adapter_weight, "transposed")


def pack_block_split3(block) -> Tuple[BlockWeights, list]:
    """The `w3` argument: the stacked bf16 weights [N, 3K], in_proj (weight and fp32 bias) with its q rows times 1/8."""
    return _pack_block_copies(block, None, "split3")


def pack_block_split3_transposed(block, adapter_weight: Optional[torch.Tensor]) -> Tuple[BlockWeights, list]:
    """The `wt3` argument: the stacked bf16 transposes [in, 3 * out]; the adapter's transpose stays fp32."""
    return _pack_block_copies(block, adapter_weight, "split3_transposed")


_BLOCK_BWD = {   # route -> (entry, its workspace-size function, error tag)
    "short": ("aaclip_block_backward", "aaclip_text_backward_workspace_bytes", "block_backward"),
    "long": ("aaclip_block_backward_long", "aaclip_block_backward_long_workspace_bytes", "block_backward"),
    "bf16x3": ("aaclip_block_backward_long_bf16x3", "aaclip_block_backward_long_bf16x3_workspace_bytes",
               "block_backward_bf16x3"),
}


def block_backward(x_in: torch.Tensor, block, B: int, L: int, heads: int, d_out: torch.Tensor, causal: bool = False,
                   adapter_weight: Optional[torch.Tensor] = None, mix: float = 0.0, need_input_grad: bool = True,
                   in_place: bool = False, long_rows: Optional[bool] = None, precision: str = "fp32"):
    """Backward of one block from its input x_in [B*L, D] -> (d x_in or None, d adapter weight [D, D] or None):
    aaclip_block_backward for L <= 128, aaclip_block_backward_long above (long_rows: see _long_rows).
    in_place: d x_in overwrites d_out.  precision "bf16x3": aaclip_block_backward_long_bf16x3 at any L."""
    precision = backward_precision_name(precision)
    require_gpu(x_in, "block_backward")
    lib = _lib.load()
    if x_in.dtype != torch.float32 or not x_in.is_contiguous() or d_out.dtype != torch.float32 or not d_out.is_contiguous():
        raise ValueError("block_backward: x_in and d_out must be contiguous fp32")
    D = x_in.shape[1]
    F = block.mlp.c_fc.weight.shape[0]
    route = _backward_route(L, long_rows, precision)
    entry, ws_bytes, tag = _BLOCK_BWD[route]
    w, refs = pack_block(block, F32, adapter_weight)
    w3, refs3 = pack_block_split3(block) if route == "bf16x3" else (None, [])
    pack_t = pack_block_split3_transposed if route == "bf16x3" else pack_block_transposed
    wt, refs_t = pack_t(block, adapter_weight) if need_input_grad else (BlockWeights(), [])
    structs = [w, wt] if w3 is None else [w, w3, wt]
    d_in = (d_out if in_place else torch.empty_like(d_out)) if need_input_grad else None
    d_aw = torch.empty(D, D, dtype=torch.float32, device=x_in.device) if adapter_weight is not None else None
    dims = (B * L, D, F) if route == "short" else (B, L, D, F)
    ws = Workspace.get(x_in.device, getattr(lib, ws_bytes)(*map(int, dims)))
    _lib.check(getattr(lib, entry)(x_in.data_ptr(), *map(C.byref, structs), float(mix), B, L, D, heads, F,
                                   ATTN_CAUSAL if causal else ATTN_FULL, d_out.data_ptr(), _ptr(d_in), _ptr(d_aw),
                                   ws.data_ptr(), ws.numel(), _stream(x_in.device)), tag)
    del refs, refs3, refs_t   # they kept the tensors behind the structs' pointers alive until the call was issued
    return d_in, d_aw


def row_head_backward(x: torch.Tensor, tokens: Optional[torch.Tensor], ln, proj: torch.Tensor, act: int, d_out: torch.Tensor,
                      n: int, T: int, mode: int, need_input_grad: bool = True):
    """Backward of row_head(kind='plain', code fp32) -> (d x [n*T, D] or None, d proj [E, D])."""
    require_gpu(x, "row_head_backward")
    lib = _lib.load()
    x, d_out = _f32c(x), _f32c(d_out)
    D = x.shape[1]
    pw = CACHE.get(proj, F32)
    pwt = CACHE.get(proj, F32, "transpose") if need_input_grad else None
    E = pw.shape[0]
    lw, lb = _f32c(ln.weight), _f32c(ln.bias)
    tk = tokens.to(device=x.device, dtype=torch.int32).contiguous() if tokens is not None else None
    d_x = torch.empty(n * T, D, dtype=torch.float32, device=x.device) if need_input_grad else None
    d_w = torch.empty(E, D, dtype=torch.float32, device=x.device)
    ws = text_backward_workspace(x.device, n * T, D, 0)
    _lib.check(lib.aaclip_row_head_backward(x.data_ptr(), _ptr(tk), lw.data_ptr(), lb.data_ptr(), pw.data_ptr(), _ptr(pwt),
                                            int(act), d_out.data_ptr(), _ptr(d_x), d_w.data_ptr(), n, T, D, E, mode,
                                            ws.data_ptr(), ws.numel(), _stream(x.device)), "row_head_backward")
    return d_x, d_w


def tap_head_backward(x: torch.Tensor, ln_post, proj_weight: Optional[torch.Tensor], act: int,
                      d_seg: Optional[torch.Tensor], det_weight: Optional[torch.Tensor] = None,
                      d_det: Optional[torch.Tensor] = None, need_input_grad: bool = True):
    """Backward of tap_head(code fp32) from the tap stream x [B, L, D] or [B*L, D] with d_seg [B, L-1, E] and / or
    d_det [B, E] -> (d x [B*L, D] or None, d proj [E, D] or None, d det [E, D] or None): aaclip_tap_head_backward.
    d_seg None: the det head alone.  need_input_grad False: the weight gradients alone, no transposed weight is read."""
    require_gpu(x, "tap_head_backward")
    lib = _lib.load()
    if d_seg is None and d_det is None:
        raise ValueError("tap_head_backward: d_seg and d_det are both None")
    if (d_det is None) != (det_weight is None):
        raise ValueError("tap_head_backward: det_weight and d_det go together")
    B = d_seg.shape[0] if d_seg is not None else d_det.shape[0]
    D = x.shape[-1]
    L = x.numel() // D // B
    x = _f32c(x).reshape(B * L, D)
    lw, lb = _f32c(ln_post.weight), _f32c(ln_post.bias)
    dev = x.device
    seg, det = d_seg is not None, d_det is not None
    E = proj_weight.shape[0] if seg else det_weight.shape[0]
    d_seg = _f32c(d_seg) if seg else None
    d_det = _f32c(d_det) if det else None
    pw = CACHE.get(proj_weight, F32) if seg else None
    pwt = CACHE.get(proj_weight, F32, "transpose") if seg and need_input_grad else None
    dw = CACHE.get(det_weight, F32) if det else None
    dwt = CACHE.get(det_weight, F32, "transpose") if det and need_input_grad else None
    d_x = torch.empty(B * L, D, dtype=torch.float32, device=dev) if need_input_grad else None
    d_pw = torch.empty(E, D, dtype=torch.float32, device=dev) if seg else None
    d_dw = torch.empty(E, D, dtype=torch.float32, device=dev) if det else None
    ws = Workspace.get(dev, lib.aaclip_tap_head_backward_workspace_bytes(int(B), int(L), int(D), int(E)))
    _lib.check(lib.aaclip_tap_head_backward(x.data_ptr(), lw.data_ptr(), lb.data_ptr(), _ptr(pw), _ptr(pwt), int(act),
                                            _ptr(d_seg), _ptr(dw), _ptr(dwt), _ptr(d_det), _ptr(d_x), _ptr(d_pw),
                                            _ptr(d_dw), B, L, D, E, ws.data_ptr(), ws.numel(), _stream(dev)),
               "tap_head_backward")
    return d_x, d_pw, d_dw


# ------------------------------------------------------------------------------------------------
# image pre-processing (reference dataset/__init__.py:150-161), Pillow-exact on the GPU
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def resample_table(in_size: int, out_size: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Host tables of one resize axis: bounds int32 [out,2], coefs int32 [out,ksize] (library-built)."""
    lib = _lib.load()
    k = lib.aaclip_resample_ksize(int(in_size), int(out_size))
    if k < 1:
        _lib.check(k, "resample_ksize")
    bounds = torch.empty(out_size, 2, dtype=torch.int32)
    coefs = torch.empty(out_size, k, dtype=torch.int32)
    _lib.check(lib.aaclip_resample_table(int(in_size), int(out_size), bounds.data_ptr(), coefs.data_ptr()),
               "resample_table")
    return bounds, coefs


_PRE_TABLES: Dict[tuple, tuple] = {}


def _normalise_lut(mean, std) -> torch.Tensor:
    # the fp32 operations of ToTensor (.div(255)) and Normalize (.sub_(mean).div_(std)), for every byte value
    v = torch.arange(256, dtype=torch.float32).div(255)
    m = torch.tensor(mean, dtype=torch.float32).view(-1, 1)
    s = torch.tensor(std, dtype=torch.float32).view(-1, 1)
    return (v.unsqueeze(0).repeat(3, 1).sub_(m).div_(s)).contiguous()


def preprocess(src_u8: torch.Tensor, img_size: int, mean=CLIP_MEAN, std=CLIP_STD) -> torch.Tensor:
    """uint8 [B,Hs,Ws,3] (HWC, on the GPU) -> fp32 [B,3,S,S]: BICUBIC resize, ToTensor, Normalize."""
    require_gpu(src_u8, "preprocess")
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 4 or src_u8.shape[-1] != 3:
        raise ValueError("preprocess expects uint8 [B, H, W, 3]")
    src_u8 = src_u8.contiguous()
    B, Hs, Ws, _ = src_u8.shape
    dev = src_u8.device
    key = (dev, Hs, Ws, img_size, tuple(mean), tuple(std))
    tabs = _PRE_TABLES.get(key)
    if tabs is None:
        hb, hk = resample_table(Ws, img_size)
        vb, vk = resample_table(Hs, img_size)
        tabs = tuple(t.to(dev) for t in (hb, hk, vb, vk, _normalise_lut(mean, std)))
        _PRE_TABLES[key] = tabs
    hb, hk, vb, vk, lut = tabs
    out = torch.empty(B, 3, img_size, img_size, device=dev, dtype=torch.float32)
    _lib.check(_lib.load().aaclip_preprocess(src_u8.data_ptr(), B, Hs, Ws, img_size, hb.data_ptr(), hk.data_ptr(),
                                             vb.data_ptr(), vk.data_ptr(), lut.data_ptr(), out.data_ptr(),
                                             _stream(dev)), "preprocess")
    return out


# ------------------------------------------------------------------------------------------------
# train-time input work (reference dataset/__init__.py:37-102): every random number is an argument
def _param(t: torch.Tensor, dtype: torch.dtype, shape: tuple, dev: torch.device, what: str) -> torch.Tensor:
    """A per-frame parameter array as the kernels read it: `dtype`, contiguous, on `dev` (host tensors are uploaded)"""
    t = torch.as_tensor(t)
    if tuple(t.shape) != shape:
        raise ValueError(f"{what} must have shape {shape}, got {tuple(t.shape)}")
    return t.to(device=dev, dtype=dtype).contiguous()


def color_jitter(src_u8: torch.Tensor, factors: torch.Tensor, apply: torch.Tensor,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [B,H,W,3] on the GPU -> uint8 [B,H,W,3]: Pillow's ImageEnhance Brightness, Contrast, Color in that order.
    factors fp32 [B,3]; apply int32 [B], bit 0 / 1 / 2 selects the brightness / contrast / saturation step.
    out: None (a new tensor) or a contiguous tensor of src's shape; `out=src_u8` works in place."""
    require_gpu(src_u8, "color_jitter")
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 4 or src_u8.shape[-1] != 3:
        raise ValueError("color_jitter expects uint8 [B, H, W, 3]")
    if out is None:
        src_u8 = src_u8.contiguous()
        out = torch.empty_like(src_u8)
    elif (not src_u8.is_contiguous() or not out.is_contiguous() or out.dtype != torch.uint8
          or out.shape != src_u8.shape or out.device != src_u8.device):
        raise ValueError("color_jitter: with out given, src and out must be contiguous uint8 tensors of one shape and device")
    B, H, W, _ = src_u8.shape
    dev = src_u8.device
    factors = _param(factors, torch.float32, (B, 3), dev, "color_jitter: factors")
    apply = _param(apply, torch.int32, (B,), dev, "color_jitter: apply")
    lib = _lib.load()
    ws = Workspace.get(dev, lib.aaclip_color_jitter_workspace_bytes(B, H, W))
    _lib.check(lib.aaclip_color_jitter(src_u8.data_ptr(), out.data_ptr(), B, H, W, factors.data_ptr(), apply.data_ptr(),
                                       ws.data_ptr(), ws.numel(), _stream(dev)), "color_jitter")
    return out


def nearest_table(in_size: int, out_size: int) -> torch.Tensor:
    """Host table of Pillow's NEAREST resize of one axis: int32 [out], the source index of every output index."""
    idx = torch.empty(out_size, dtype=torch.int32)
    _lib.check(_lib.load().aaclip_nearest_table(int(in_size), int(out_size), idx.data_ptr()), "nearest_table")
    return idx


_NEAREST_TABLES: Dict[tuple, tuple] = {}


def mask_preprocess(mask_u8: torch.Tensor, img_size: int, normal: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [B,Hm,Wm] on the GPU -> fp32 [B,1,S,S] of 0 / 1: Resize((S,S), NEAREST), ToTensor, != 0.
    normal [B] (any integer / bool dtype) or None: a set entry gives an all-zero mask, its source is not read."""
    require_gpu(mask_u8, "mask_preprocess")
    if mask_u8.dtype != torch.uint8 or mask_u8.dim() != 3:
        raise ValueError("mask_preprocess expects uint8 [B, H, W]")
    mask_u8 = mask_u8.contiguous()
    B, Hm, Wm = mask_u8.shape
    dev = mask_u8.device
    key = (dev, Hm, Wm, img_size)
    tabs = _NEAREST_TABLES.get(key)
    if tabs is None:
        tabs = (nearest_table(Wm, img_size).to(dev), nearest_table(Hm, img_size).to(dev))
        _NEAREST_TABLES[key] = tabs
    if normal is not None:
        normal = _param(normal, torch.int32, (B,), dev, "mask_preprocess: normal")
    out = torch.empty(B, 1, img_size, img_size, device=dev, dtype=torch.float32)
    _lib.check(_lib.load().aaclip_mask_preprocess(mask_u8.data_ptr(), B, Hm, Wm, img_size, tabs[0].data_ptr(),
                                                  tabs[1].data_ptr(), _ptr(normal), out.data_ptr(), _stream(dev)),
               "mask_preprocess")
    return out


def augment_geometric(image: torch.Tensor, mask: torch.Tensor, angle_deg: torch.Tensor, shift: torch.Tensor,
                      flags: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """image fp32 [B,3,S,S], mask fp32 [B,1,S,S] on the GPU -> (image, mask) after, per frame, rotation by angle_deg
    (flags bit 0), shift by shift[b] = (tx, ty) (bit 1), horizontal flip (bit 2), vertical flip (bit 3), in that order:
    nearest sampling, zero fill.  angle_deg fp32 [B], shift int32 [B,2], flags int32 [B]."""
    require_gpu(image, "augment_geometric")
    require_gpu(mask, "augment_geometric")
    if (image.dtype != torch.float32 or image.dim() != 4 or image.shape[1] != 3 or image.shape[2] != image.shape[3]
            or mask.dtype != torch.float32 or tuple(mask.shape) != (image.shape[0], 1) + tuple(image.shape[2:])):
        raise ValueError("augment_geometric expects fp32 image [B, 3, S, S] and fp32 mask [B, 1, S, S]")
    image, mask = image.contiguous(), mask.contiguous()
    B, _, S, _ = image.shape
    dev = image.device
    angle_deg = _param(angle_deg, torch.float32, (B,), dev, "augment_geometric: angle_deg")
    shift = _param(shift, torch.int32, (B, 2), dev, "augment_geometric: shift")
    flags = _param(flags, torch.int32, (B,), dev, "augment_geometric: flags")
    image_out, mask_out = torch.empty_like(image), torch.empty_like(mask)
    _lib.check(_lib.load().aaclip_augment_geometric(image.data_ptr(), mask.data_ptr(), B, S, angle_deg.data_ptr(),
                                                    shift.data_ptr(), flags.data_ptr(), image_out.data_ptr(),
                                                    mask_out.data_ptr(), _stream(dev)), "augment_geometric")
    return image_out, mask_out


def train_preprocess(frames_u8: torch.Tensor, masks_u8: torch.Tensor, normal: torch.Tensor, params: dict,
                     img_size: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The reference's train-time transform of one group of equally sized frames (dataset/__init__.py:37-102) for GIVEN
    random numbers: colour jitter -> BICUBIC resize, ToTensor, Normalize (preprocess, unchanged) on the frames, NEAREST
    resize and != 0 on the masks, then rotation / shift / flips of both together.
    frames_u8 uint8 [B,H,W,3], masks_u8 uint8 [B,Hm,Wm], normal [B] (set: the frame has no mask), all on the GPU;
    params: the dict of dataset.draw_augment_params -> (image fp32 [B,3,S,S], mask fp32 [B,1,S,S])."""
    frames = color_jitter(frames_u8, params["color_factors"], params["color_apply"])
    image = preprocess(frames, img_size)
    mask = mask_preprocess(masks_u8, img_size, normal)
    return augment_geometric(image, mask, params["angle"], params["shift"], params["flags"])


# ------------------------------------------------------------------------------------------------
# exact AUROC / AP of one class on the device (csrc/metrics.hip; forward_utils.metrics_eval_device)
METRICS_MAX_N = 2 ** 31 - 1
CURVE_RECORD_WORDS = 6          # int64 words: num, P, N, groups, ap (fp64 bits), scores outside [0, 1] of a packed sort
CurveMetrics = collections.namedtuple("CurveMetrics", "auroc ap P N image_max num groups")


def _metrics_inputs(scores: torch.Tensor, labels: Optional[torch.Tensor], what: str):
    require_gpu(scores, what)
    if labels is not None:
        require_gpu(labels, what)
    if scores.dtype != torch.float32 or (labels is not None and labels.dtype != torch.uint8):
        raise ValueError(f"{what} expects fp32 scores and uint8 labels")
    scores = scores.contiguous().view(-1)
    if labels is not None:
        labels = labels.contiguous().view(-1)
        if labels.numel() != scores.numel() or labels.device != scores.device:
            raise ValueError(f"{what}: scores and labels must have one size and device")
    if not 2 <= scores.numel() <= METRICS_MAX_N:
        raise ValueError(f"{what}: 2 .. 2^31 - 1 scores, got {scores.numel()}")
    return scores, labels


def metrics_range(scores: torch.Tensor, labels: Optional[torch.Tensor] = None, per_image: int = 0):
    """-> (record, image_max): the device record of aaclip_metrics_range (int64 [3]: min | max as two fp32, non-finite
    count, positive count; metrics_range_host reads it) and the fp32 maximum of every `per_image` scores (None for 0)."""
    scores, labels = _metrics_inputs(scores, labels, "metrics_range")
    n, dev = scores.numel(), scores.device
    if per_image < 0 or (per_image and n % per_image):
        raise ValueError(f"metrics_range: {n} scores are no multiple of per_image = {per_image}")
    lib = _lib.load()
    record = torch.empty(3, dtype=torch.int64, device=dev)
    image_max = torch.empty(n // per_image, dtype=torch.float32, device=dev) if per_image else None
    ws = Workspace.get(dev, lib.aaclip_metrics_range_workspace_bytes(n, per_image))
    _lib.check(lib.aaclip_metrics_range(scores.data_ptr(), _ptr(labels), n, per_image, _ptr(image_max), record.data_ptr(),
                                        ws.data_ptr(), ws.numel(), _stream(dev)), "metrics_range")
    return record, image_max


def metrics_range_host(record: torch.Tensor) -> dict:
    """The range record on the host (one synchronising copy of 24 bytes)."""
    r = record.cpu()
    mn, mx = r[:1].view(torch.float32).tolist()
    return {"min": mn, "max": mx, "nonfinite": int(r[1]), "positives": int(r[2])}


def metrics_normalise(scores: torch.Tensor, record: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(x - min) / (max - min) in fp32 with numpy's bits when the record's max != 1, else x; decided on the device."""
    require_gpu(scores, "metrics_normalise")
    if scores.dtype != torch.float32 or record.dtype != torch.int64 or record.numel() != 3 or not record.is_cuda:
        raise ValueError("metrics_normalise expects fp32 scores and the record of metrics_range")
    scores = scores.contiguous()
    if out is None:
        out = torch.empty_like(scores)
    elif out.dtype != torch.float32 or out.shape != scores.shape or not out.is_contiguous() or out.device != scores.device:
        raise ValueError("metrics_normalise: out must be a contiguous fp32 tensor of scores' shape and device")
    _lib.check(_lib.load().aaclip_metrics_normalise(scores.data_ptr(), out.data_ptr(), scores.numel(), record.data_ptr(),
                                                    _stream(scores.device)), "metrics_normalise")
    return out


def metrics_sort(scores: torch.Tensor, labels: torch.Tensor, packed: bool, out_of_range: Optional[torch.Tensor] = None):
    """-> (keys, labels_sorted, out_of_range): the ascending keys of aaclip_metrics_sort as int32 [n] (read them as
    uint32), the labels in their order (None when packed: bit 0 of the key) and the device count (int64 [1]) of
    scores outside [0, 1] that a packed sort met."""
    scores, labels = _metrics_inputs(scores, labels, "metrics_sort")
    if labels is None:
        raise ValueError("metrics_sort needs labels")
    n, dev = scores.numel(), scores.device
    lib = _lib.load()
    keys = torch.empty(n, dtype=torch.int32, device=dev)
    labels_sorted = None if packed else torch.empty(n, dtype=torch.uint8, device=dev)
    if out_of_range is None:
        out_of_range = torch.empty(1, dtype=torch.int64, device=dev)
    ws = Workspace.get(dev, lib.aaclip_metrics_sort_workspace_bytes(n))
    _lib.check(lib.aaclip_metrics_sort(scores.data_ptr(), labels.data_ptr(), n, int(bool(packed)), keys.data_ptr(),
                                       _ptr(labels_sorted), out_of_range.data_ptr(), ws.data_ptr(), ws.numel(),
                                       _stream(dev)), "metrics_sort")
    return keys, labels_sorted, out_of_range


def metrics_curve(keys: torch.Tensor, labels_sorted: Optional[torch.Tensor], packed: bool,
                  record: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Sorted keys -> the device record (int64 [CURVE_RECORD_WORDS]; words 0..4 are written: num, P, N, groups, ap bits)."""
    require_gpu(keys, "metrics_curve")
    if keys.dtype != torch.int32 or keys.dim() != 1 or not keys.is_contiguous() or not 2 <= keys.numel() <= METRICS_MAX_N:
        raise ValueError("metrics_curve expects the int32 [n] keys of metrics_sort")
    if not packed and (labels_sorted is None or labels_sorted.dtype != torch.uint8 or labels_sorted.numel() != keys.numel()
                       or not labels_sorted.is_contiguous() or labels_sorted.device != keys.device):
        raise ValueError("metrics_curve: keys without a packed label need the uint8 [n] labels of metrics_sort")
    n, dev = keys.numel(), keys.device
    if record is None:
        record = torch.zeros(CURVE_RECORD_WORDS, dtype=torch.int64, device=dev)
    lib = _lib.load()
    ws = Workspace.get(dev, lib.aaclip_metrics_curve_workspace_bytes(n))
    _lib.check(lib.aaclip_metrics_curve(keys.data_ptr(), None if packed else labels_sorted.data_ptr(), n,
                                        int(bool(packed)), record.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)),
               "metrics_curve")
    return record


def _curve_record_arg(record: Optional[torch.Tensor], what: str) -> None:
    if record is not None and (record.dtype != torch.int64 or record.numel() != CURVE_RECORD_WORDS or not record.is_cuda
                               or not record.is_contiguous()):
        raise ValueError(f"{what}: record must be a contiguous int64 [{CURVE_RECORD_WORDS}] device tensor")


def _sorted_curve(scores: torch.Tensor, labels: torch.Tensor, per_image: int, record: Optional[torch.Tensor],
                  normalise: bool, what: str, f1_record: Optional[torch.Tensor] = None):
    """The body of curve_metrics and f1max_metrics: the range, the checks, ONE sort, the curve sums and -- when
    f1_record (int64 [F1MAX_RECORD_WORDS], device) is given -- the F1-max argmax over the same sorted keys.
    -> (CurveMetrics, range record on the device, the f1max record on the host or None)"""
    n = scores.numel()
    rng, image_max = metrics_range(scores, labels, per_image)
    r = metrics_range_host(rng)
    if r["nonfinite"]:
        raise ValueError(f"{what}: {r['nonfinite']} of {n} scores are not finite")
    if normalise and r["max"] == r["min"]:
        raise ValueError(f"{what}: all scores are equal (max == min): the min-max normalisation divides by zero")
    if r["positives"] == 0 or r["positives"] == n:
        raise ValueError(f"{what}: only one class present in the labels; AUROC and AP are not defined")
    norm = metrics_normalise(scores, rng) if normalise else scores
    if normalise and image_max is not None:
        metrics_normalise(image_max, rng, out=image_max)
    # the label rides in the key where every sorted score lies in [0, 1]: normalised, or passed through inside it
    packed = (normalise and r["max"] != 1.0) or (r["min"] >= 0.0 and r["max"] <= 1.0)
    if record is None:
        record = torch.zeros(CURVE_RECORD_WORDS, dtype=torch.int64, device=scores.device)
    keys, labels_sorted, _ = metrics_sort(norm, labels, packed, out_of_range=record[CURVE_RECORD_WORDS - 1:])
    del norm
    metrics_curve(keys, labels_sorted, packed, record)
    if f1_record is not None:
        metrics_f1max(keys, labels_sorted, packed, f1_record)
    h = record.cpu()
    num, P, N, groups, _, outside = (int(v) for v in h)
    if outside:
        raise RuntimeError(f"{what}: {outside} normalised scores fell outside [0, 1]")
    assert P == r["positives"] and P + N == n, (P, N, r, n)
    curve = CurveMetrics(num / (2 * P * N), float(h[4:5].view(torch.float64)), P, N, image_max, num, groups)
    return curve, rng, (None if f1_record is None else f1_record.cpu())


def curve_metrics(scores: torch.Tensor, labels: torch.Tensor, per_image: int = 0,
                  record: Optional[torch.Tensor] = None, normalise: bool = True) -> CurveMetrics:
    """sklearn's roc_auc_score and average_precision_score of the min-max normalised scores (reference
    forward_utils.py:246-253,288-296), exactly, on the device: scores fp32, labels uint8 (0 / non-zero), any shape of one
    size.  -> CurveMetrics(auroc, ap, P, N, image_max, num, groups): auroc = num / (2 P N) with the integer numerator
    num, ap the fp64 sum over the `groups` distinct scores, image_max the fp32 device tensor of the NORMALISED maximum
    of every `per_image` scores (None for per_image = 0).
    Raises ValueError before anything is sorted when a score is not finite, when max == min (the reference divides by
    zero there) or when the labels hold one class only (sklearn raises).  record: an int64 [CURVE_RECORD_WORDS] device
    tensor to receive the device record (it is not written when the call raises).
    normalise=False takes the scores as they are (metrics_eval's image scores are normalised before they are combined
    with the map maxima, not after); equal scores are then one tie group, not an error."""
    scores, labels = _metrics_inputs(scores, labels, "curve_metrics")
    if labels is None:
        raise ValueError("curve_metrics needs labels")
    _curve_record_arg(record, "curve_metrics")
    return _sorted_curve(scores, labels, per_image, record, normalise, "curve_metrics")[0]


# ------------------------------------------------------------------------------------------------
# bootstrap of AUROC / AP over the images of one class (csrc/bootstrap.hip; forward_utils.bootstrap_eval_device)
BOOTSTRAP_RECORD_WORDS = 4      # int64 words per replicate: num, P, N, ap (fp64 bits)
BootstrapCurves = collections.namedtuple("BootstrapCurves", "num P N ap valid auroc")


def bootstrap_max_images() -> int:
    """The largest number of images of one bootstrap_curves call (the weight table of a replicate block lives in LDS)."""
    return int(_lib.load().aaclip_bootstrap_max_images())


def bootstrap_counts_tensor(counts, dev: torch.device) -> torch.Tensor:
    """counts [R, images] (a host array or a tensor anywhere) -> a contiguous uint8 device tensor; ValueError for a
    negative count or one above 255."""
    c = torch.as_tensor(counts)
    if c.dim() != 2 or c.shape[0] < 1 or c.shape[1] < 1 or c.dtype.is_floating_point or c.dtype == torch.bool:
        raise ValueError("bootstrap counts must be an integer array [R, images]")
    if c.dtype != torch.uint8:
        if int(c.min()) < 0 or int(c.max()) > 255:
            raise ValueError("bootstrap counts must lie in 0 .. 255 (they are stored as uint8)")
        c = c.to(torch.uint8)
    return c.to(dev).contiguous()


def bootstrap_curves(keys: torch.Tensor, payload_sorted: torch.Tensor, counts, packed: bool = False) -> torch.Tensor:
    """The weighted curve sums of every replicate: keys int32 [n] ascending and payload_sorted int32 [n] = image << 1 |
    label in their order (metrics_sort_pairs of the values image << 1 | label), counts [R, images] in 0 .. 255.
    -> records int64 [R, BOOTSTRAP_RECORD_WORDS] on the device: num, P, N, ap (fp64 bits); an invalid replicate (P == 0 or
    N == 0) has num = 0 and ap = 0.  ValueError before any launch for more images than bootstrap_max_images(), for a
    payload that names an image outside the counts, and for a replicate whose weighted size reaches 2^31.
    packed: must be False -- the pair sort's keys are unpacked, the label rides in the payload."""
    require_gpu(keys, "bootstrap_curves")
    require_gpu(payload_sorted, "bootstrap_curves")
    if packed:
        raise ValueError("bootstrap_curves takes the unpacked keys of metrics_sort_pairs")
    n, dev = keys.numel(), keys.device
    if keys.dtype != torch.int32 or keys.dim() != 1 or not keys.is_contiguous() or not 1 <= n <= METRICS_MAX_N:
        raise ValueError("bootstrap_curves expects the int32 [n] keys of metrics_sort_pairs")
    if (payload_sorted.dtype != torch.int32 or payload_sorted.shape != keys.shape or not payload_sorted.is_contiguous()
            or payload_sorted.device != dev):
        raise ValueError("bootstrap_curves expects the int32 [n] sorted payload of metrics_sort_pairs")
    counts = bootstrap_counts_tensor(counts, dev)
    R, images = (int(v) for v in counts.shape)
    lib = _lib.load()
    if images > lib.aaclip_bootstrap_max_images():
        raise ValueError(f"bootstrap_curves: {images} images, this build supports {lib.aaclip_bootstrap_max_images()} "
                         "per call")
    image = payload_sorted >> 1
    if int(image.min()) < 0 or int(image.max()) >= images:
        raise ValueError(f"bootstrap_curves: the payload names an image outside 0 .. {images - 1}")
    elements = torch.bincount(image, minlength=images)
    heaviest = int((counts.to(torch.int64) * elements[None, :]).sum(dim=1).max())
    if heaviest >= 2 ** 31:
        raise ValueError(f"bootstrap_curves: a replicate weighs {heaviest} elements; the sums need less than 2^31")
    records = torch.empty(R, BOOTSTRAP_RECORD_WORDS, dtype=torch.int64, device=dev)
    ws = Workspace.get(dev, lib.aaclip_bootstrap_workspace_bytes(n, images, R))
    plan = _lib.BootstrapPlan(n=n, images=images, replicates=R, stream=_stream(dev))
    _lib.check(lib.aaclip_bootstrap_curves(C.byref(plan), keys.data_ptr(), payload_sorted.data_ptr(), counts.data_ptr(),
                                           records.data_ptr(), ws.data_ptr(), ws.numel()), "bootstrap_curves")
    return records


def bootstrap_records_host(records: torch.Tensor) -> BootstrapCurves:
    """The records of bootstrap_curves on the host (one synchronising copy): numpy arrays over the replicates; auroc =
    num / (2 P N) in fp64, 0 where the replicate is invalid."""
    h = records.cpu()
    num, P, N = (h[:, k].numpy().copy() for k in range(3))
    ap = h[:, 3].contiguous().view(torch.float64).numpy().copy()
    valid = (P > 0) & (N > 0)
    auroc = num.astype("float64") / (2.0 * P * N).clip(min=1.0)
    auroc[~valid] = 0.0
    return BootstrapCurves(num, P, N, ap, valid, auroc)


def bootstrap_metrics(scores: torch.Tensor, labels: torch.Tensor, per_image: int, counts,
                      normalise: bool = True) -> BootstrapCurves:
    """AUROC / AP of every bootstrap replicate over images: scores fp32 and labels uint8 of images * per_image elements,
    image i owning the elements [i * per_image, (i + 1) * per_image); counts [R, images].  The scores are those
    curve_metrics sorts (min-max normalised over the whole class when normalise: the range is NOT recomputed per
    replicate), sorted ONCE with the payload image << 1 | label; bootstrap_curves does the rest.  per_image = 1 serves
    the image scores.  -> BootstrapCurves(num, P, N, ap, valid, auroc) of numpy arrays [R].
    Raises ValueError where curve_metrics does (non-finite scores, max == min under normalise, one class only)."""
    scores, labels = _metrics_inputs(scores, labels, "bootstrap_metrics")
    if labels is None:
        raise ValueError("bootstrap_metrics needs labels")
    n, dev = scores.numel(), scores.device
    if per_image < 1 or n % per_image:
        raise ValueError(f"bootstrap_metrics: {n} scores are no multiple of per_image = {per_image}")
    images = n // per_image
    counts = bootstrap_counts_tensor(counts, dev)
    if counts.shape[1] != images:
        raise ValueError(f"bootstrap_metrics: counts of {counts.shape[1]} images for {images} images")
    if images > bootstrap_max_images():
        raise ValueError(f"bootstrap_metrics: {images} images, this build supports {bootstrap_max_images()} per call")
    rng, _ = metrics_range(scores, labels)
    r = metrics_range_host(rng)
    if r["nonfinite"]:
        raise ValueError(f"bootstrap_metrics: {r['nonfinite']} of {n} scores are not finite")
    if normalise and r["max"] == r["min"]:
        raise ValueError("bootstrap_metrics: all scores are equal (max == min): the min-max normalisation divides by zero")
    if r["positives"] == 0 or r["positives"] == n:
        raise ValueError("bootstrap_metrics: only one class present in the labels; AUROC and AP are not defined")
    norm = metrics_normalise(scores, rng) if normalise else scores
    payload = (torch.arange(n, dtype=torch.int32, device=dev).div_(per_image, rounding_mode="floor") << 1) | (labels != 0)
    keys, payload_sorted = metrics_sort_pairs(norm, payload.to(torch.int32))
    del norm, payload
    return bootstrap_records_host(bootstrap_curves(keys, payload_sorted, counts))


# ------------------------------------------------------------------------------------------------
# exact F1-max and its operating point (csrc/metrics.hip; forward_utils.f1max_eval_device), masks at a threshold
F1MAX_RECORD_WORDS = 7          # int64 words: tp, fp, P, N, groups, start index, key (low half) | fp32 threshold bits (high)
THRESHOLD_RECORD_WORDS = 4      # int64 words: tp, fp, fn, tn
F1Max = collections.namedtuple("F1Max", "f1 threshold tp fp fn precision recall groups")


def f1max_from_counts(tp: int, fp: int, P: int, threshold: float, groups: int) -> F1Max:
    """The F1Max of integer counts: f1 = 2 tp / (2 tp + fp + fn) is ONE division of Python integers, so the host and the
    device path, which agree on the integers, agree on its bits."""
    tp, fp, fn = int(tp), int(fp), int(P) - int(tp)
    return F1Max(2 * tp / (2 * tp + fp + fn), float(threshold), tp, fp, fn, tp / (tp + fp) if tp + fp else 0.0,
                 tp / (tp + fn), int(groups))


def f1max_record_host(record: torch.Tensor) -> dict:
    """The f1max record on the host (one synchronising copy of 56 bytes)."""
    h = record.cpu()
    tp, fp, P, N, groups, start, last = (int(v) for v in h)
    return {"tp": tp, "fp": fp, "P": P, "N": N, "groups": groups, "start": start, "key": last & 0xFFFFFFFF,
            "threshold": float(h[6:7].view(torch.float32)[1])}


def metrics_f1max(keys: torch.Tensor, labels_sorted: Optional[torch.Tensor], packed: bool,
                  record: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Sorted keys (metrics_sort's) -> the device record of aaclip_metrics_f1max (int64 [F1MAX_RECORD_WORDS];
    f1max_record_host reads it): the tie group with the largest F1, the higher score among exactly equal ones."""
    require_gpu(keys, "metrics_f1max")
    if keys.dtype != torch.int32 or keys.dim() != 1 or not keys.is_contiguous() or not 2 <= keys.numel() <= METRICS_MAX_N:
        raise ValueError("metrics_f1max expects the int32 [n] keys of metrics_sort")
    if not packed and (labels_sorted is None or labels_sorted.dtype != torch.uint8 or labels_sorted.numel() != keys.numel()
                       or not labels_sorted.is_contiguous() or labels_sorted.device != keys.device):
        raise ValueError("metrics_f1max: keys without a packed label need the uint8 [n] labels of metrics_sort")
    n, dev = keys.numel(), keys.device
    if record is None:
        record = torch.zeros(F1MAX_RECORD_WORDS, dtype=torch.int64, device=dev)
    elif (record.dtype != torch.int64 or record.numel() != F1MAX_RECORD_WORDS or record.device != dev
          or not record.is_contiguous()):
        raise ValueError(f"metrics_f1max: record must be a contiguous int64 [{F1MAX_RECORD_WORDS}] tensor on the keys' device")
    lib = _lib.load()
    ws = Workspace.get(dev, lib.aaclip_metrics_f1max_workspace_bytes(n))
    _lib.check(lib.aaclip_metrics_f1max(keys.data_ptr(), None if packed else labels_sorted.data_ptr(), n,
                                        int(bool(packed)), record.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)),
               "metrics_f1max")
    return record


def threshold_record(threshold: float, dev: torch.device) -> torch.Tensor:
    """A device f1max record that carries nothing but the fp32 threshold (what metrics_threshold reads)"""
    host = torch.zeros(F1MAX_RECORD_WORDS, dtype=torch.int64)
    host[6:7].view(torch.float32)[1] = float(threshold)
    return host.to(dev)


def metrics_threshold(scores: torch.Tensor, threshold, labels: Optional[torch.Tensor] = None, per_image: int = 0,
                      range_record: Optional[torch.Tensor] = None, mask: bool = True, totals: bool = True):
    """-> (mask, image_counts, totals) of the fp32 scores at a threshold: mask uint8 in scores' shape, 1 where the
    score -- normalised on the fly with range_record (metrics_range's) when that is given -- is >= the threshold;
    image_counts int32 [n / per_image, 4] = tp, fp, fn, tn of every image when labels and per_image > 0 are given,
    else None; totals int64 [4] on the device = tp, fp, fn, tn (without labels: fp = flagged, tn = the rest).
    threshold: the device record of metrics_f1max (read on the device, nothing synchronises) or a number.
    mask=False / totals=False leave that output out (None)."""
    shape = scores.shape
    scores, labels = _metrics_inputs(scores, labels, "metrics_threshold")
    n, dev = scores.numel(), scores.device
    if per_image < 0 or (per_image and n % per_image):
        raise ValueError(f"metrics_threshold: {n} scores are no multiple of per_image = {per_image}")
    if torch.is_tensor(threshold):
        if (threshold.dtype != torch.int64 or threshold.numel() != F1MAX_RECORD_WORDS or threshold.device != dev
                or not threshold.is_contiguous()):
            raise ValueError("metrics_threshold: a tensor threshold must be the int64 record of metrics_f1max on the "
                             "scores' device")
        f1_record = threshold
    else:
        f1_record = threshold_record(threshold, dev)
    if range_record is not None and (range_record.dtype != torch.int64 or range_record.numel() != 3
                                     or range_record.device != dev):
        raise ValueError("metrics_threshold: range_record must be the int64 [3] record of metrics_range")
    counts = labels is not None and per_image > 0
    if not (mask or totals or counts):
        raise ValueError("metrics_threshold: nothing to compute (no mask, no totals, no per-image counts)")
    lib = _lib.load()
    out_mask = torch.empty(n, dtype=torch.uint8, device=dev) if mask else None
    out_counts = torch.empty(n // per_image, 4, dtype=torch.int32, device=dev) if counts else None
    out_totals = torch.empty(THRESHOLD_RECORD_WORDS, dtype=torch.int64, device=dev) if totals else None
    ws = Workspace.get(dev, lib.aaclip_metrics_threshold_workspace_bytes(n, per_image))
    _lib.check(lib.aaclip_metrics_threshold(scores.data_ptr(), _ptr(labels), n, per_image, _ptr(range_record),
                                            f1_record.data_ptr(), _ptr(out_mask), _ptr(out_counts), _ptr(out_totals),
                                            ws.data_ptr(), ws.numel(), _stream(dev)), "metrics_threshold")
    return (out_mask.view(shape) if mask else None), out_counts, out_totals


def f1max_metrics(scores: torch.Tensor, labels: torch.Tensor, per_image: int = 0, normalise: bool = True,
                  records: Optional[dict] = None):
    """curve_metrics and the exact F1-max from ONE sort: -> (CurveMetrics, F1Max(f1, threshold, tp, fp, fn, precision,
    recall, groups)).  F1-max is the largest 2 tp / (2 tp + fp + fn) over every distinct threshold, compared in integers;
    among thresholds of exactly equal F1 the highest; threshold is in the units that were sorted (normalised ones when
    normalise) and predicted = score >= threshold.  The arguments, checks and ValueErrors are curve_metrics'.
    records: a dict that receives the device records "range" and "f1max" (what metrics_threshold takes)."""
    scores, labels = _metrics_inputs(scores, labels, "f1max_metrics")
    if labels is None:
        raise ValueError("f1max_metrics needs labels")
    f1_record = torch.zeros(F1MAX_RECORD_WORDS, dtype=torch.int64, device=scores.device)
    curve, rng, h = _sorted_curve(scores, labels, per_image, None, normalise, "f1max_metrics", f1_record)
    tp, fp, P, N, groups = (int(v) for v in h[:5])
    assert (P, N, groups) == (curve.P, curve.N, curve.groups), (h, curve)
    if records is not None:
        records["range"], records["f1max"] = rng, f1_record
    return curve, f1max_from_counts(tp, fp, P, float(h[6:7].view(torch.float32)[1]), groups)


# ------------------------------------------------------------------------------------------------
# per-region overlap (AUPRO) of one class on the device (csrc/regions.hip; forward_utils.pro_eval_device)
PRO_RECORD_WORDS = 5            # int64 words: aupro (fp64 bits), regions, normal pixels, groups, y at the limit (fp64 bits)
ProMetrics = collections.namedtuple("ProMetrics", "aupro regions normal groups")


def _mask_images(mask: torch.Tensor, what: str):
    """uint8 device mask [N, H, W] (or [N, 1, H, W], or [H, W]) -> (contiguous mask, images, H, W)"""
    require_gpu(mask, what)
    if mask.dtype != torch.uint8 or mask.dim() < 2:
        raise ValueError(f"{what} expects a uint8 mask of [images, H, W]")
    H, W = int(mask.shape[-2]), int(mask.shape[-1])
    n = mask.numel()
    if H < 1 or W < 1 or not 2 <= n <= METRICS_MAX_N:
        raise ValueError(f"{what}: 2 .. 2^31 - 1 pixels in images of at least 1 x 1, got {tuple(mask.shape)}")
    return mask.contiguous(), n // (H * W), H, W


def metrics_regions(mask: torch.Tensor, connectivity: int = 8):
    """-> (region, area, record): the connected components of the non-zero pixels of every image of the uint8 mask
    [N, H, W].  region (int32, mask's shape; read it as uint32): 0 for a normal pixel, else 1 + the flat index of the
    first pixel, in row-major order over the whole tensor, of the pixel's component; area (int32): the component's
    pixel count, 0 for a normal pixel; record: int64 [3] on the device = regions, anomalous pixels, normal pixels."""
    mask, images, H, W = _mask_images(mask, "metrics_regions")
    if connectivity not in (4, 8):
        raise ValueError(f"metrics_regions: connectivity must be 4 or 8, got {connectivity}")
    dev = mask.device
    lib = _lib.load()
    region = torch.empty(mask.shape, dtype=torch.int32, device=dev)
    area = torch.empty(mask.shape, dtype=torch.int32, device=dev)
    record = torch.empty(3, dtype=torch.int64, device=dev)
    ws = Workspace.get(dev, lib.aaclip_metrics_regions_workspace_bytes(images, H, W))
    _lib.check(lib.aaclip_metrics_regions(mask.data_ptr(), images, H, W, connectivity, region.data_ptr(), area.data_ptr(),
                                          record.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)), "metrics_regions")
    return region, area, record


def metrics_sort_pairs(scores: torch.Tensor, values: torch.Tensor):
    """-> (keys, values_sorted): the ascending unpacked keys of the fp32 scores as int32 [n] (read them as uint32) and
    the int32 values in their order; equal keys keep their input order."""
    scores, _ = _metrics_inputs(scores, None, "metrics_sort_pairs")
    require_gpu(values, "metrics_sort_pairs")
    if values.dtype != torch.int32 or values.numel() != scores.numel() or values.device != scores.device:
        raise ValueError("metrics_sort_pairs expects int32 values of the scores' size and device")
    values = values.contiguous().view(-1)
    n, dev = scores.numel(), scores.device
    lib = _lib.load()
    keys = torch.empty(n, dtype=torch.int32, device=dev)
    values_sorted = torch.empty(n, dtype=torch.int32, device=dev)
    ws = Workspace.get(dev, lib.aaclip_metrics_sort_pairs_workspace_bytes(n))
    _lib.check(lib.aaclip_metrics_sort_pairs(scores.data_ptr(), values.data_ptr(), n, keys.data_ptr(),
                                             values_sorted.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)),
               "metrics_sort_pairs")
    return keys, values_sorted


def metrics_pro_curve(keys: torch.Tensor, areas_sorted: torch.Tensor, regions_record: torch.Tensor, fpr_limit: float,
                      record: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Sorted (key, area) pairs and the record of metrics_regions -> the device record (int64 [PRO_RECORD_WORDS]: aupro
    bits, regions, normal pixels, groups, bits of y at the limit)."""
    require_gpu(keys, "metrics_pro_curve")
    n, dev = keys.numel(), keys.device
    if keys.dtype != torch.int32 or keys.dim() != 1 or not keys.is_contiguous() or not 2 <= n <= METRICS_MAX_N:
        raise ValueError("metrics_pro_curve expects the int32 [n] keys of metrics_sort_pairs")
    if (areas_sorted.dtype != torch.int32 or areas_sorted.shape != keys.shape or not areas_sorted.is_contiguous()
            or areas_sorted.device != dev):
        raise ValueError("metrics_pro_curve expects the int32 [n] sorted areas of metrics_sort_pairs")
    if regions_record.dtype != torch.int64 or regions_record.numel() != 3 or regions_record.device != dev:
        raise ValueError("metrics_pro_curve expects the int64 [3] record of metrics_regions")
    if not 0.0 < float(fpr_limit) <= 1.0:
        raise ValueError(f"metrics_pro_curve: fpr_limit must lie in (0, 1], got {fpr_limit}")
    if record is None:
        record = torch.zeros(PRO_RECORD_WORDS, dtype=torch.int64, device=dev)
    lib = _lib.load()
    ws = Workspace.get(dev, lib.aaclip_metrics_pro_curve_workspace_bytes(n))
    _lib.check(lib.aaclip_metrics_pro_curve(keys.data_ptr(), areas_sorted.data_ptr(), n, regions_record.data_ptr(),
                                            float(fpr_limit), record.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)),
               "metrics_pro_curve")
    return record


def pro_metrics(scores: torch.Tensor, mask: torch.Tensor, fpr_limit: float = 0.3, connectivity: int = 8,
                normalise: bool = True) -> ProMetrics:
    """The per-region overlap curve of the min-max normalised scores integrated up to the false-positive rate fpr_limit
    and divided by it (AUPRO), exactly, on the device: forward_utils.pro_eval's definition over every distinct score.
    scores fp32 and mask uint8 (non-zero = anomalous) [N, H, W].  -> ProMetrics(aupro, regions, normal, groups).
    Raises ValueError before anything is sorted when the mask holds no region or no normal pixel, when a score is not
    finite or when max == min; normalise=False takes the scores as they are (equal scores are then one tie group)."""
    mask, images, H, W = _mask_images(mask, "pro_metrics")
    scores, _ = _metrics_inputs(scores, None, "pro_metrics")
    if scores.numel() != mask.numel() or scores.device != mask.device:
        raise ValueError("pro_metrics: scores and mask must have one size and device")
    if not 0.0 < float(fpr_limit) <= 1.0:
        raise ValueError(f"pro_metrics: fpr_limit must lie in (0, 1], got {fpr_limit}")
    n = scores.numel()
    _, area, regions_record = metrics_regions(mask, connectivity)
    rng, _ = metrics_range(scores)
    R, _, normal = (int(v) for v in regions_record.cpu())
    r = metrics_range_host(rng)
    if R == 0 or normal == 0:
        raise ValueError(f"pro_metrics: {R} regions and {normal} normal pixels; the PRO curve needs both")
    if r["nonfinite"]:
        raise ValueError(f"pro_metrics: {r['nonfinite']} of {n} scores are not finite")
    if normalise and r["max"] == r["min"]:
        raise ValueError("pro_metrics: all scores are equal (max == min): the min-max normalisation divides by zero")
    norm = metrics_normalise(scores, rng) if normalise else scores
    keys, areas_sorted = metrics_sort_pairs(norm, area)
    del norm, area
    h = metrics_pro_curve(keys, areas_sorted, regions_record, fpr_limit).cpu()
    assert int(h[1]) == R and int(h[2]) == normal, (h, R, normal)
    return ProMetrics(float(h[0:1].view(torch.float64)), R, normal, int(h[3]))


# ------------------------------------------------------------------------------------------------
# defect instances at an operating point (csrc/region_table.hip; forward_utils.defects_eval_device)
REGION_ROW_WORDS = 12           # int32 words of a row, in REGION_ROW_FIELDS' order; `peak` holds fp32 bits
REGION_ROW_FIELDS = ("image", "label", "first", "area", "x0", "y0", "x1", "y1", "peak_x", "peak_y", "peak", "overlap")
REGION_TABLE_RECORD_WORDS = 4   # int64 words: rows kept, regions seen, kept regions with overlap > 0, rows dropped
DEFECTS_RECORD_WORDS = 6        # int64 words: predicted regions, predicted hit, gt regions, gt hit, images, images with >= 1
RegionTable = collections.namedtuple("RegionTable", "rows image_offsets record kept_mask")
Defects = collections.namedtuple("Defects", "predicted truth record mask")


def region_table(region: torch.Tensor, area: torch.Tensor, scores: torch.Tensor, other: Optional[torch.Tensor] = None,
                 range_record: Optional[torch.Tensor] = None, min_area: int = 1, kept_mask: bool = False,
                 regions=None) -> RegionTable:
    """-> RegionTable(rows, image_offsets, record, kept_mask), device tensors: the regions of metrics_regions (its
    `region` and `area`, [N, H, W]) with at least min_area pixels as rows int32 [R, 12] (REGION_ROW_FIELDS) in canonical
    order -- ascending (image, first pixel), scipy's label order; image_offsets int32 [N + 1], the rows in front of
    every image; record int64 [4] = rows kept, regions seen, kept regions that overlap `other`, rows dropped.
    scores fp32 of the same size: `peak` is the largest score of the region, normalised on the fly with range_record
    (metrics_range's) when that is given, (peak_x, peak_y) the lowest flat index that attains it.  other: a uint8 mask of
    the same size whose non-zero pixels are counted in `overlap`.  kept_mask=True also returns the uint8 mask of the
    kept regions' pixels.
    regions: the record of metrics_regions (one synchronising copy of 24 bytes sizes `rows`) or the region count as a
    number; None takes the most regions the images can hold (every other pixel), which is safe and large.  `rows` is cut to
    the rows kept (with the record and min_area = 1 that is every row, and nothing more is read back).  Raises
    RuntimeError if the record reports dropped rows (a count that was too small)."""
    require_gpu(region, "region_table")
    shape, dev = region.shape, region.device
    if region.dtype != torch.int32 or region.dim() < 2 or not 2 <= region.numel() <= METRICS_MAX_N:
        raise ValueError("region_table expects the int32 [images, H, W] region map of metrics_regions")
    n, H, W = region.numel(), int(shape[-2]), int(shape[-1])
    images = n // (H * W)
    for name, t, dt in (("area", area, torch.int32), ("scores", scores, torch.float32), ("other", other, torch.uint8)):
        if t is not None and (t.dtype != dt or t.numel() != n or t.device != dev):
            raise ValueError(f"region_table: {name} must be a {dt} tensor of the region map's size and device")
    if range_record is not None and (range_record.dtype != torch.int64 or range_record.numel() != 3
                                     or range_record.device != dev):
        raise ValueError("region_table: range_record must be the int64 [3] record of metrics_range")
    if int(min_area) < 1:
        raise ValueError(f"region_table: min_area must be at least 1, got {min_area}")
    exact = torch.is_tensor(regions)
    if exact:
        if regions.dtype != torch.int64 or regions.numel() != 3:
            raise ValueError("region_table: regions must be the int64 [3] record of metrics_regions or a number")
        capacity = int(regions.cpu()[0])
    else:
        capacity = images * ((H * W + 1) // 2) if regions is None else int(regions)
    if capacity < 0:
        raise ValueError(f"region_table: a negative region count, {capacity}")
    region, area, scores = region.contiguous(), area.contiguous(), scores.contiguous()
    other = None if other is None else other.contiguous()
    lib = _lib.load()
    rows = torch.empty(capacity, REGION_ROW_WORDS, dtype=torch.int32, device=dev)
    offsets = torch.empty(images + 1, dtype=torch.int32, device=dev)
    record = torch.empty(REGION_TABLE_RECORD_WORDS, dtype=torch.int64, device=dev)
    kept = torch.empty(shape, dtype=torch.uint8, device=dev) if kept_mask else None
    ws = Workspace.get(dev, lib.aaclip_region_table_workspace_bytes(images, H, W))
    _lib.check(lib.aaclip_region_table(region.data_ptr(), area.data_ptr(), scores.data_ptr(), _ptr(range_record),
                                       _ptr(other), images, H, W, int(min_area), capacity,
                                       rows.data_ptr() if capacity else None, offsets.data_ptr(), _ptr(kept),
                                       record.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)), "region_table")
    if not (exact and int(min_area) == 1):      # with the regions record and no filter every row is written: R = capacity
        h = record.cpu()
        if int(h[3]):
            raise RuntimeError(f"region_table: {int(h[3])} of {int(h[0])} rows were dropped: the region count "
                               f"{capacity} is too small for this region map")
        rows = rows[:int(h[0])]
    return RegionTable(rows, offsets, record, kept)


def region_rows_per_image(rows, image_offsets) -> list:
    """Host arrays of a region table (rows int32 [R, 12], offsets [N + 1]) -> a list per image of dicts with
    REGION_ROW_FIELDS' keys (without "image"), `peak` as a float, in canonical order."""
    import numpy as np
    rows = np.asarray(rows).reshape(-1, REGION_ROW_WORDS)
    peaks = np.ascontiguousarray(rows[:, 10]).view(np.float32)
    names = [(c, k) for c, k in enumerate(REGION_ROW_FIELDS) if k not in ("image", "peak")]
    out = []
    for i in range(len(image_offsets) - 1):
        span = range(int(image_offsets[i]), int(image_offsets[i + 1]))
        assert all(int(rows[j, 0]) == i for j in span), "a row outside its image's offsets"
        out.append([dict({k: int(rows[j, c]) for c, k in names}, peak=float(peaks[j])) for j in span])
    return out


def region_table_host(table: RegionTable) -> list:
    """The device table on the host (region_rows_per_image of it); raises if the record reports dropped rows."""
    record = table.record.cpu()
    if int(record[3]):
        raise RuntimeError(f"region_table_host: {int(record[3])} rows were dropped")
    return region_rows_per_image(table.rows.cpu().numpy()[:int(record[0])], table.image_offsets.cpu().numpy())


def defects_at_threshold(scores: torch.Tensor, threshold, range_record: Optional[torch.Tensor], gt_mask=None,
                         min_area: int = 1, connectivity: int = 8) -> Defects:
    """The defect instances of fp32 maps [N, H, W] at an operating point, on the device: metrics_threshold gives the
    predicted mask (threshold: the device record of metrics_f1max, read on the device, or a number; scores normalised on
    the fly with range_record when given), metrics_regions labels it, region_table lists the regions of at least
    min_area pixels with other = gt_mask.  With gt_mask (uint8, non-zero = anomalous) the ground truth is labelled too
    and tabulated against the KEPT predicted mask, which says which true regions were found.
    -> Defects(predicted, truth, record, mask): two RegionTables (truth None without gt_mask), the device record int64
    [6] = predicted regions, predicted regions that touch ground truth, gt regions, gt regions that were hit, images,
    images with at least one predicted region; mask = the kept predicted uint8 mask."""
    require_gpu(scores, "defects_at_threshold")
    if scores.dtype != torch.float32 or scores.dim() < 2:
        raise ValueError("defects_at_threshold expects fp32 maps of [images, H, W]")
    dev, shape = scores.device, scores.shape
    if gt_mask is not None:
        require_gpu(gt_mask, "defects_at_threshold")
        if gt_mask.dtype != torch.uint8 or gt_mask.numel() != scores.numel() or gt_mask.device != dev:
            raise ValueError("defects_at_threshold: gt_mask must be a uint8 tensor of the maps' size and device")
        gt_mask = gt_mask.contiguous().view(shape)
    predicted_mask = metrics_threshold(scores, threshold, range_record=range_record, totals=False)[0]
    region, area, regions_record = metrics_regions(predicted_mask, connectivity)
    predicted = region_table(region, area, scores, other=gt_mask, range_record=range_record, min_area=min_area,
                             kept_mask=True, regions=regions_record)
    del region, area
    images = predicted.image_offsets.numel() - 1
    with_any = (predicted.image_offsets[1:] != predicted.image_offsets[:-1]).sum()
    record = torch.zeros(DEFECTS_RECORD_WORDS, dtype=torch.int64, device=dev)
    record[0], record[1], record[4], record[5] = predicted.record[0], predicted.record[2], images, with_any
    truth = None
    if gt_mask is not None:
        region, area, regions_record = metrics_regions(gt_mask, connectivity)
        truth = region_table(region, area, scores, other=predicted.kept_mask, range_record=range_record,
                             regions=regions_record)
        record[2], record[3] = truth.record[0], truth.record[2]
    return Defects(predicted, truth, record, predicted.kept_mask)


# ------------------------------------------------------------------------------------------------
# IQM side branch (reference model/iqm.py, model/adapter.py:186-269, test_last.py:102-147): thin wrappers of the C ABI
def gemm(code: int, epi: int, a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor,
         act: int = 0) -> torch.Tensor:
    """aaclip_gemm on prepared operands: a [M, K] and w [N, K] in the compute dtype, bias fp32 [N] or None,
    out [M, N] (16-bit for EPI_BIAS / EPI_BIAS_GELU, fp32 for EPI_ACT_F32)."""
    M = a.shape[0]
    N = w.shape[0]
    if code == F16X2:                                # split rows hold 4 bytes per element; lda / ldc count halves
        lda = a.shape[1] * a.element_size() // 2
        K = lda // 2
        ldc = out.shape[1] * out.element_size() // 2 if out.dtype != torch.float32 else out.shape[1]
    else:
        lda = K = a.shape[1]
        ldc = out.shape[1]
    _lib.check(_lib.load().aaclip_gemm(code, epi, a.data_ptr(), lda, w.data_ptr(), _ptr(bias), out.data_ptr(),
                                       ldc, M, N, K, int(act), 0, 1.0, _stream(a.device)), "gemm")
    return out


def small_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, B: int, nq: int, Lk: int, heads: int,
                    kv_code: int) -> torch.Tensor:
    """softmax(q k^T / sqrt(hd)) v for a handful of queries (reference model/iqm.py:108-139).  q fp32 [B*nq, D];
    k, v [B*Lk, D] in the kv dtype -> fp32 [B*nq, D]."""
    D = q.shape[-1]
    hd = D // heads
    out = torch.empty(B * nq, D, dtype=torch.float32, device=q.device)
    _lib.check(_lib.load().aaclip_small_attention(kv_code, q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, nq,
                                                  Lk, heads, hd, 1.0 / (hd ** 0.5), _stream(q.device)), "small_attention")
    return out


def cross_rows(qt: torch.Tensor, x: torch.Tensor, B: int, R: int, Lk: int, x_code: int) -> torch.Tensor:
    """out[b, r] = softmax_j(qt[b, r] . x[b, j]) . x[b]: R effective queries per image over the raw rows x [B*Lk, Dk]
    (reference model/iqm.py:108-139 after folding W_k into the query and W_v behind the weighted sum; include/aaclip.h).
    qt fp32 [B*R, Dk] -> fp32 [B*R, Dk]."""
    lib = _lib.load()
    Dk = x.shape[-1]
    out = torch.empty(B * R, Dk, dtype=torch.float32, device=x.device)
    ws = Workspace.get(x.device, lib.aaclip_cross_rows_workspace_bytes(B, R, Lk, Dk) + 256)
    _lib.check(lib.aaclip_cross_rows(x_code, qt.data_ptr(), x.data_ptr(), out.data_ptr(), B, R, Lk, Dk, ws.data_ptr(),
                                     ws.numel(), _stream(x.device)), "cross_rows")
    return out


CROSS_ROWS_BACKWARD_MAX_SLICES = 128   # csrc/kernels.h CRB_MAX_SLICES: key slices per image of aaclip_cross_rows_backward


def cross_rows_backward(qt: torch.Tensor, x: torch.Tensor, d_out: torch.Tensor, B: int, R: int, Lk: int, x_code: int,
                        act: int = _lib.ACT_NONE, need_qt: bool = True, need_x: bool = True,
                        d_x: Optional[torch.Tensor] = None):
    """Backward of cross_rows from d_out [B*R, Dk] -> (d qt fp32 [B*R, Dk] or None, d x fp32 [B*Lk, Dk] or None):
    aaclip_cross_rows_backward.  qt fp32 and x [B*Lk, Dk] (x_code) as the forward read them.  act: the activation whose
    OUTPUT x is; d x is then the gradient of the pre-activation rows.  d_x given (contiguous fp32 [B*Lk, Dk]): the
    gradient is ADDED into it (accumulate) and it is returned."""
    require_gpu(x, "cross_rows_backward")
    lib = _lib.load()
    if not (need_qt or need_x):
        raise ValueError("cross_rows_backward: nothing to compute")
    Dk = x.shape[-1]
    if not x.is_contiguous() or x.dtype != _TORCH_DT[x_code] or x.numel() != B * Lk * Dk:
        raise ValueError("cross_rows_backward: x must be contiguous [B*Lk, Dk] in the dtype x_code names")
    qt, d_out = _f32c(qt), _f32c(d_out)
    if qt.numel() != B * R * Dk or d_out.numel() != B * R * Dk:
        raise ValueError("cross_rows_backward: qt and d_out must be [B*R, Dk]")
    accumulate = d_x is not None
    if accumulate and (d_x.dtype != torch.float32 or not d_x.is_contiguous() or d_x.numel() != B * Lk * Dk or not need_x):
        raise ValueError("cross_rows_backward: d_x must be contiguous fp32 [B*Lk, Dk] (and need_x set)")
    d_qt = torch.empty(B * R, Dk, dtype=torch.float32, device=x.device) if need_qt else None
    if need_x and d_x is None:
        d_x = torch.empty(B * Lk, Dk, dtype=torch.float32, device=x.device)
    ws = Workspace.get(x.device, lib.aaclip_cross_rows_backward_workspace_bytes(B, R, Lk, Dk))
    _lib.check(lib.aaclip_cross_rows_backward(x_code, qt.data_ptr(), x.data_ptr(), d_out.data_ptr(), _ptr(d_qt),
                                              _ptr(d_x) if need_x else None, int(act), int(accumulate), B, R, Lk, Dk,
                                              ws.data_ptr(), ws.numel(), _stream(x.device)), "cross_rows_backward")
    return d_qt, (d_x if need_x else None)


def cross_rows_levels(qt: torch.Tensor, levels, B: int, R: int, rows_per_image: int, row0: int, Lk: int,
                      Dk: int) -> torch.Tensor:
    """include/aaclip.h aaclip_cross_rows_levels.  qt fp32 [B*R, nseg*Dk]; levels = row buffers, one per segment: fp16 /
    bf16 [B*rows_per_image, Dk], or uint8 split8 rows [B*rows_per_image, 4*Dk] (their fp16 halves are read)."""
    require_gpu(qt, "cross_rows_levels")
    lib = _lib.load()
    nseg = len(levels)
    xc, ldx = _level_rows(levels, "cross_rows_levels")
    if levels[0].device != qt.device:
        raise ValueError("cross_rows_levels: the level buffers must agree in dtype, shape and device")
    if qt.shape != (B * R, nseg * Dk) or qt.dtype != torch.float32 or not qt.is_contiguous():
        raise ValueError("cross_rows_levels: qt must be contiguous fp32 [B*R, nseg*Dk]")
    ptrs = (C.c_void_p * nseg)(*[x.data_ptr() for x in levels])
    out = torch.empty(B * R, nseg * Dk, dtype=torch.float32, device=qt.device)
    ws = Workspace.get(qt.device, lib.aaclip_cross_rows_levels_workspace_bytes(B, nseg, Lk, Dk) + 256)
    _lib.check(lib.aaclip_cross_rows_levels(xc, qt.data_ptr(), ptrs, nseg, out.data_ptr(), B, R, rows_per_image, row0, Lk,
                                            Dk, ldx, ws.data_ptr(), ws.numel(), _stream(qt.device)), "cross_rows_levels")
    return out


def _level_rows(levels, what: str):
    """-> (x dtype code, row stride in elements) of the level buffers of cross_rows_levels: fp16 / bf16 rows, or uint8
    split8 rows whose fp16 halves are read"""
    x0 = levels[0]
    if x0.dtype == torch.uint8:
        xc, ldx = _lib.F16, x0.shape[1] // 2
    elif x0.dtype in (torch.float16, torch.bfloat16):
        xc, ldx = {torch.float16: F16, torch.bfloat16: BF16}[x0.dtype], x0.shape[1]
    else:
        raise ValueError(f"{what}: the level buffers must be fp16, bf16 or uint8 split8 rows")
    for x in levels:
        if x.dtype != x0.dtype or x.shape != x0.shape or not x.is_contiguous() or x.device != x0.device:
            raise ValueError(f"{what}: the level buffers must agree in dtype, shape and device")
    return xc, ldx


def cross_rows_levels_backward(qt: torch.Tensor, levels, d_out: torch.Tensor, B: int, R: int, rows_per_image: int,
                               row0: int, Lk: int, Dk: int, need_qt: bool = True, need_x: bool = True, d_x=None,
                               overwrite: bool = False):
    """Backward of cross_rows_levels from d_out [B*R, nseg*Dk] -> (d qt fp32 [B*R, nseg*Dk] or None, d x: a list of fp32
    [B*rows_per_image, Dk] per level or None): aaclip_cross_rows_levels_backward.  qt and levels as the forward took
    them.  d_x given (a list of contiguous fp32 [B*rows_per_image, Dk]): the gradient is ADDED into its key rows
    (accumulate; with overwrite it replaces them) and the list is returned; its other rows are left as they are.
    Buffers made here are zero outside the key rows."""
    require_gpu(qt, "cross_rows_levels_backward")
    lib = _lib.load()
    if not (need_qt or need_x):
        raise ValueError("cross_rows_levels_backward: nothing to compute")
    nseg = len(levels)
    xc, ldx = _level_rows(levels, "cross_rows_levels_backward")
    rows = levels[0].shape[0]
    qt, d_out = _f32c(qt), _f32c(d_out)
    if qt.numel() != B * R * nseg * Dk or d_out.numel() != qt.numel() or rows != B * rows_per_image:
        raise ValueError("cross_rows_levels_backward: qt and d_out must be [B*R, nseg*Dk], the levels [B*rows_per_image, .]")
    accumulate = d_x is not None and not overwrite
    if d_x is not None and (not need_x or len(d_x) != nseg or any(
            g.dtype != torch.float32 or not g.is_contiguous() or g.shape != (rows, Dk) or g.device != qt.device
            for g in d_x)):
        raise ValueError("cross_rows_levels_backward: d_x must be one contiguous fp32 [B*rows_per_image, Dk] per level "
                         "(and need_x set)")
    d_qt = torch.empty(B * R, nseg * Dk, dtype=torch.float32, device=qt.device) if need_qt else None
    if need_x and d_x is None:
        d_x = [torch.zeros(rows, Dk, dtype=torch.float32, device=qt.device) for _ in range(nseg)]
    xp = (C.c_void_p * nseg)(*[x.data_ptr() for x in levels])
    gp = (C.c_void_p * nseg)(*[g.data_ptr() for g in d_x]) if need_x else None
    ws = Workspace.get(qt.device, lib.aaclip_cross_rows_levels_backward_workspace_bytes(B, R, nseg, Lk, Dk))
    _lib.check(lib.aaclip_cross_rows_levels_backward(xc, qt.data_ptr(), xp, nseg, d_out.data_ptr(), _ptr(d_qt), gp,
                                                     int(accumulate), B, R, rows_per_image, row0, Lk, Dk, ldx,
                                                     ws.data_ptr(), ws.numel(), _stream(qt.device)),
               "cross_rows_levels_backward")
    return d_qt, (list(d_x) if need_x else None)


def head_expand(q: torch.Tensor, heads: int, scale: float, code: int) -> torch.Tensor:
    """q fp32 [rows, D] -> [rows*H, D] in the compute dtype: row (r, h) = q[r] * scale on head h's columns, else zero."""
    rows, D = q.shape
    out = torch.empty(rows * heads, D, dtype=_TORCH_DT[code], device=q.device)
    _lib.check(_lib.load().aaclip_head_expand(code, q.data_ptr(), out.data_ptr(), rows, heads, D, float(scale),
                                              _stream(q.device)), "head_expand")
    return out


def head_diag(full: torch.Tensor, heads: int) -> torch.Tensor:
    """full fp32 [rows*H, D] -> [rows, D]: the head-diagonal blocks (row (r, h), columns of head h)."""
    D = full.shape[-1]
    rows = full.shape[0] // heads
    out = torch.empty(rows, D, dtype=torch.float32, device=full.device)
    _lib.check(_lib.load().aaclip_head_diag(full.data_ptr(), out.data_ptr(), rows, heads, D, _stream(full.device)),
               "head_diag")
    return out


def residual_layernorm(a: torch.Tensor, b: Optional[torch.Tensor], ln, eps: float) -> torch.Tensor:
    """LayerNorm(a + b) (reference model/iqm.py:150-154); fp32 [rows, D]."""
    rows, D = a.shape
    out = torch.empty_like(a)
    w, bias = _f32c(ln.weight), _f32c(ln.bias)
    _lib.check(_lib.load().aaclip_residual_layernorm(a.data_ptr(), _ptr(b), w.data_ptr(), bias.data_ptr(), out.data_ptr(),
                                                     rows, D, float(eps), _stream(a.device)), "residual_layernorm")
    return out


def combine3(a: torch.Tensor, b: Optional[torch.Tensor], c: Optional[torch.Tensor], wa: float, wb: float,
             wc: float) -> torch.Tensor:
    out = torch.empty_like(a)
    _lib.check(_lib.load().aaclip_combine3(a.data_ptr(), _ptr(b), _ptr(c), float(wa), float(wb), float(wc), out.data_ptr(),
                                           a.numel(), _stream(a.device)), "combine3")
    return out


def linear_smallk(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], out_code: int) -> torch.Tensor:
    """y = x W^T + b for in_features <= 4 -> [R, N] in the compute dtype."""
    x = _f32c(x)
    K = x.shape[-1]
    x2 = x.reshape(-1, K)
    w, b = _f32c(weight), (_f32c(bias) if bias is not None else None)
    out = torch.empty(x2.shape[0], w.shape[0], dtype=_TORCH_DT[out_code], device=x.device)
    _lib.check(_lib.load().aaclip_linear_smallk(out_code, x2.data_ptr(), w.data_ptr(), _ptr(b), out.data_ptr(), x2.shape[0],
                                                w.shape[0], K, _stream(x.device)), "linear_smallk")
    return out


# ------------------------------------------------------------------------------------------------
# backward building blocks of the IQM branch's query side (include/aaclip.h, csrc/iqm_query_backward.hip): fp32
SMALL_ATTENTION_BACKWARD_MAX_KEYS = 256   # csrc/kernels.h SAB_MAXK


def small_attention_backward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, d_out: torch.Tensor, B: int, nq: int,
                             Lk: int, heads: int, need_q: bool = True, need_k: bool = True, need_v: bool = True):
    """Backward of small_attention for fp32 k / v -> (d q [B*nq, D], d k [B*Lk, D], d v [B*Lk, D]), None where not
    needed: aaclip_small_attention_backward."""
    require_gpu(q, "small_attention_backward")
    if not (need_q or need_k or need_v):
        raise ValueError("small_attention_backward: nothing to compute")
    q, k, v, d_out = _f32c(q), _f32c(k), _f32c(v), _f32c(d_out)
    D = q.shape[-1]
    hd = D // heads
    d_q = torch.empty_like(q) if need_q else None
    d_k = torch.empty_like(k) if need_k else None
    d_v = torch.empty_like(v) if need_v else None
    _lib.check(_lib.load().aaclip_small_attention_backward(q.data_ptr(), k.data_ptr(), v.data_ptr(), d_out.data_ptr(),
                                                           _ptr(d_q), _ptr(d_k), _ptr(d_v), B, nq, Lk, heads, hd,
                                                           1.0 / (hd ** 0.5), _stream(q.device)),
               "small_attention_backward")
    return d_q, d_k, d_v


def layernorm_param_grad(x: torch.Tensor, d_y: torch.Tensor, eps: float):
    """(d weight [D], d bias [D]) of y = LayerNorm(x) over fp32 rows [rows, D]: aaclip_layernorm_param_grad."""
    require_gpu(x, "layernorm_param_grad")
    lib = _lib.load()
    x, d_y = _f32c(x), _f32c(d_y)
    D = x.shape[-1]
    rows = x.numel() // D
    d_w = torch.empty(D, dtype=torch.float32, device=x.device)
    d_b = torch.empty_like(d_w)
    ws = Workspace.get(x.device, lib.aaclip_layernorm_param_grad_workspace_bytes(rows, D))
    _lib.check(lib.aaclip_layernorm_param_grad(x.data_ptr(), d_y.data_ptr(), d_w.data_ptr(), d_b.data_ptr(), rows, D,
                                               float(eps), ws.data_ptr(), ws.numel(), _stream(x.device)),
               "layernorm_param_grad")
    return d_w, d_b


def bias_grad(dz: torch.Tensor, N: Optional[int] = None) -> torch.Tensor:
    """db[n] = sum_r dz[r, n] over the first N columns (default: all) of contiguous fp32 dz [rows, ldz]."""
    require_gpu(dz, "bias_grad")
    lib = _lib.load()
    dz = _f32c(dz)
    rows, ldz = dz.shape
    N = ldz if N is None else int(N)
    db = torch.empty(N, dtype=torch.float32, device=dz.device)
    ws = Workspace.get(dz.device, lib.aaclip_bias_grad_workspace_bytes(rows, N))
    _lib.check(lib.aaclip_bias_grad(dz.data_ptr(), ldz, db.data_ptr(), rows, N, ws.data_ptr(), ws.numel(),
                                    _stream(dz.device)), "bias_grad")
    return db


def act_backward(act: int, zy: torch.Tensor, d_y: torch.Tensor, in_place: bool = False) -> torch.Tensor:
    """d z = d y * act': ACT_GELU from the pre-activation zy, ACT_RELU from the activation's output zy.
    in_place: d z overwrites d_y (contiguous fp32)."""
    require_gpu(zy, "act_backward")
    zy = _f32c(zy)
    if in_place:
        if d_y.dtype != torch.float32 or not d_y.is_contiguous():
            raise ValueError("act_backward: in_place needs a contiguous fp32 d_y")
    else:
        d_y = _f32c(d_y)
    if d_y.numel() != zy.numel():
        raise ValueError("act_backward: zy and d_y must have the same number of elements")
    d_z = d_y if in_place else torch.empty_like(d_y)
    _lib.check(_lib.load().aaclip_act_backward(int(act), zy.data_ptr(), d_y.data_ptr(), d_z.data_ptr(), zy.numel(),
                                               _stream(zy.device)), "act_backward")
    return d_z


def linear_smallk_backward(x: torch.Tensor, d_y: torch.Tensor):
    """(d weight [N, K], d bias [N]) of y = x W^T + b for in_features K <= 4; x [..., K], d_y [R, N] fp32."""
    require_gpu(d_y, "linear_smallk_backward")
    lib = _lib.load()
    x, d_y = _f32c(x), _f32c(d_y)
    K = x.shape[-1]
    R, N = d_y.shape
    if x.numel() != R * K:
        raise ValueError("linear_smallk_backward: x must hold one row of K values per row of d_y")
    d_w = torch.empty(N, K, dtype=torch.float32, device=d_y.device)
    d_b = torch.empty(N, dtype=torch.float32, device=d_y.device)
    ws = Workspace.get(d_y.device, lib.aaclip_linear_smallk_backward_workspace_bytes(R, N, K))
    _lib.check(lib.aaclip_linear_smallk_backward(x.data_ptr(), d_y.data_ptr(), d_w.data_ptr(), d_b.data_ptr(), R, N, K,
                                                 ws.data_ptr(), ws.numel(), _stream(d_y.device)),
               "linear_smallk_backward")
    return d_w, d_b


def drop_cls_rows(src: torch.Tensor, dst: torch.Tensor, B: int, L: int, row_off: int, code: int) -> None:
    """src [B*L, E] -> rows 1.. of every image into dst [B, rows_per_image, E] at row_off."""
    E = src.shape[-1]
    _lib.check(_lib.load().aaclip_drop_cls_rows(code, src.data_ptr(), dst.data_ptr(), B, L, E, dst.shape[1], row_off,
                                                _stream(src.device)), "drop_cls_rows")


def iqm_map(seg_tokens: Sequence[torch.Tensor], queries: torch.Tensor, img_size: int, base: Optional[torch.Tensor] = None,
            w_base: float = 0.0, w_iqm: float = 1.0) -> torch.Tensor:
    """reference test_last.py:102-147 -> [B, S, S] = w_base * base + w_iqm * sum over levels of the upsampled
    sigmoid(cos(f, q_abnormal) - cos(f, q_normal))."""
    lib = _lib.load()
    segs = [_f32c(s) for s in seg_tokens]
    require_gpu(segs[0], "iqm_map")
    B, P, E = segs[0].shape
    g = int(round(P ** 0.5))
    if g * g != P:
        raise AssertionError(f"L={P} is not a perfect square")         # reference test_last.py:125
    q = _f32c(queries)
    if q.shape != (B, 2, E):
        raise ValueError("queries must be [B, 2, E] (normal, abnormal)")
    out = torch.empty(B, img_size, img_size, dtype=torch.float32, device=segs[0].device)
    bs = _f32c(base) if base is not None else None
    if bs is not None and bs.shape != out.shape:
        raise ValueError("base map must be [B, S, S]")
    ws = Workspace.get(segs[0].device, len(segs) * B * P * 4 + 256)
    arr = (C.c_void_p * len(segs))(*[s.data_ptr() for s in segs])
    _lib.check(lib.aaclip_iqm_map(arr, len(segs), q.data_ptr(), _ptr(bs), out.data_ptr(), B, g, E, img_size, float(w_base),
                                  float(w_iqm), ws.data_ptr(), ws.numel(), _stream(out.device)), "iqm_map")
    return out


# ------------------------------------------------------------------------------- few-shot support bank (csrc/support.hip)
SUPPORT_FP32, SUPPORT_FP16 = _lib.SUPPORT_FP32, _lib.SUPPORT_FP16
SUPPORT_FORMS = {"fp16": SUPPORT_FP16, "fp32": SUPPORT_FP32}
SUPPORT_OPERAND_EXP = 4          # csrc/support_pack.h: the fp16 form's bank rows are fp16(v * 2^4)
SupportBank = collections.namedtuple("SupportBank", "rows form patches shots")
SupportBank.__doc__ = """rows: per tap level the bank [N, E] in the form's layout (fp16 of v * 2^4, or fp32), N = shots *
patches in (shot, patch) order; form: SUPPORT_FP16 / SUPPORT_FP32; patches: rows per image; shots: images in the bank."""


def support_form(form) -> int:
    """'fp16' / 'fp32' (or the code itself) -> SUPPORT_FP16 / SUPPORT_FP32"""
    if isinstance(form, str):
        form = SUPPORT_FORMS.get(form.lower())
    if form not in (SUPPORT_FP16, SUPPORT_FP32):
        raise ValueError("support form must be 'fp16' or 'fp32'")
    return int(form)


def support_bank_rows(rows: torch.Tensor, form) -> torch.Tensor:
    """fp32 rows [N, E] -> the bank of one level in the form's layout (aaclip_support_bank_rows)"""
    form = support_form(form)
    r = _f32c(rows)
    require_gpu(r, "support_bank_rows")
    if r.dim() != 2:
        raise ValueError("support_bank_rows expects rows of [N, E]")
    N, E = r.shape
    out = torch.empty(N, E, dtype=torch.float16 if form == SUPPORT_FP16 else torch.float32, device=r.device)
    _lib.check(_lib.load().aaclip_support_bank_rows(r.data_ptr(), N, E, form, out.data_ptr(), _stream(r.device)),
               "support_bank_rows")
    return out


def support_bank(seg_tokens_per_image_batch, form) -> SupportBank:
    """The bank of k normal images: seg_tokens_per_image_batch is a sequence of batches, each the per-level list of unit
    fp32 seg tokens [b, P, E] that AdaptedCLIP.forward returns (one batch's list is accepted too).  The images are
    concatenated in order, so bank row shot * P + patch is that patch of that image."""
    form = support_form(form)
    batches = list(seg_tokens_per_image_batch)
    if not batches:
        raise ValueError("support_bank: no images")
    if torch.is_tensor(batches[0]):
        batches = [batches]
    levels = len(batches[0])
    if levels < 1 or any(len(b) != levels for b in batches):
        raise ValueError("support_bank: every batch must hold the same tap levels")
    require_gpu(batches[0][0], "support_bank")
    P, E = batches[0][0].shape[1:]
    shots = sum(int(b[0].shape[0]) for b in batches)
    rows = []
    for l in range(levels):
        parts = [_f32c(b[l]) for b in batches]
        if any(p.dim() != 3 or tuple(p.shape[1:]) != (P, E) for p in parts):
            raise ValueError("support_bank: seg tokens must be [b, P, E] with one P and E")
        rows.append(support_bank_rows(torch.cat(parts, dim=0).reshape(shots * P, E), form))
    return SupportBank(rows, form, int(P), shots)


def support_nearest(q: torch.Tensor, bank_level: torch.Tensor, form=None, want_idx: bool = True):
    """-> (cos fp32 [M], idx int32 [M]): for every row of q ([M, E], or [B, P, E] taken as B * P rows) the largest inner
    product with a row of bank_level (one entry of SupportBank.rows; the form is read off its dtype unless given) and
    the lowest bank row that attains it.  want_idx=False returns idx = None."""
    form = (SUPPORT_FP16 if bank_level.dtype == torch.float16 else SUPPORT_FP32) if form is None else support_form(form)
    qq = _f32c(q)
    require_gpu(qq, "support_nearest")
    require_gpu(bank_level, "support_nearest")
    qq = qq.reshape(-1, qq.shape[-1])
    M, E = qq.shape
    want = torch.float16 if form == SUPPORT_FP16 else torch.float32
    if bank_level.dim() != 2 or bank_level.shape[1] != E or bank_level.dtype != want or bank_level.device != qq.device:
        raise ValueError(f"support_nearest: the bank must be a {want} tensor [N, {E}] on the queries' device")
    bank_level = bank_level.contiguous()
    lib = _lib.load()
    dev = qq.device
    cos = torch.empty(M, dtype=torch.float32, device=dev)
    idx = torch.empty(M, dtype=torch.int32, device=dev) if want_idx else None
    N = bank_level.shape[0]
    ws = Workspace.get(dev, max(256, lib.aaclip_support_nearest_workspace_bytes(M, N, E, form)))
    _lib.check(lib.aaclip_support_nearest(qq.data_ptr(), M, bank_level.data_ptr(), N, E, form, cos.data_ptr(), _ptr(idx),
                                          ws.data_ptr(), ws.numel(), _stream(dev)), "support_nearest")
    return cos, idx


def support_map_from_cos(cos_levels: Sequence[torch.Tensor], B: int, img_size: int, ksize: int, sigma: float,
                         base: Optional[torch.Tensor] = None, weight: float = 50.0) -> torch.Tensor:
    """The map stage alone: per level best_cos [B * g * g] -> [B, S, S] = base + weight * sum over levels of
    upsample(blur(1 - best_cos)) with anomaly_map's blur, upsample and level order (aaclip_support_map)."""
    cs = [_f32c(c).reshape(-1) for c in cos_levels]
    require_gpu(cs[0], "support_map")
    dev = cs[0].device
    P = cs[0].numel() // B
    g = int(round(P ** 0.5))
    if g * g != P or any(c.numel() != B * P for c in cs):
        raise ValueError(f"support_map: {cs[0].numel()} cosines are not {B} square grids")
    out = torch.empty(B, img_size, img_size, dtype=torch.float32, device=dev)
    bs = _f32c(base) if base is not None else None
    if bs is not None and (bs.shape != out.shape or bs.device != dev):
        raise ValueError("base map must be [B, S, S] on the tokens' device")
    ws = Workspace.get(dev, len(cs) * B * P * 4 + 256)
    arr = (C.c_void_p * len(cs))(*[c.data_ptr() for c in cs])
    _lib.check(_lib.load().aaclip_support_map(arr, len(cs), _ptr(bs), float(weight), out.data_ptr(), B, g, img_size,
                                              int(ksize), float(sigma), ws.data_ptr(), ws.numel(), _stream(dev)),
               "support_map")
    return out


def support_map(seg_tokens: Sequence[torch.Tensor], bank: SupportBank, img_size: int, ksize: int, sigma: float,
                base: Optional[torch.Tensor] = None, weight: float = 50.0, nearest: Optional[list] = None) -> torch.Tensor:
    """-> [B, S, S] = base + weight * sum over levels of upsample(blur(d_l)), d_l = 1 - (largest cosine of every patch to
    the level's bank rows) on the g x g grid, not clamped; base=None counts as 0.  nearest: a list that receives the
    int32 [B, P] index of the nearest bank row per level (shot, patch = divmod(index, bank.patches))."""
    segs = list(seg_tokens)
    if len(segs) != len(bank.rows):
        raise ValueError(f"support_map: {len(segs)} levels of tokens for a bank of {len(bank.rows)}")
    B, P = segs[0].shape[:2]
    cos = []
    for s, rows in zip(segs, bank.rows):
        c, i = support_nearest(s, rows, bank.form, want_idx=nearest is not None)
        cos.append(c)
        if nearest is not None:
            nearest.append(i.reshape(B, P))
    return support_map_from_cos(cos, B, img_size, ksize, sigma, base, weight)


# ------------------------------------------------------------------------------- coreset of the bank (csrc/coreset.hip)
CORESET_SCALE_EXP = 14           # csrc/coreset_pack.h: rows are quantised to int16 of v * 2^14
CORESET_NORM2_LIMIT = 1 << 29    # the selection's precondition on every norm2
CoresetBank = collections.namedtuple("CoresetBank", "rows form patches shots index radius2 dim")
CoresetBank.__doc__ = """SupportBank's fields with SupportBank's meaning -- rows holds only the kept rows, patches and
shots describe the FULL bank -- and: index: per level an int32 device tensor, for each kept row its row in the full bank,
in pick order; radius2: per level the host uint32 array of covering radii squared (entry t with t picks, in units of
2^-28: radius2 / 2^29 is the cosine distance on unit rows); dim: the width the selection ran on (0: the rows' own)."""


def coreset_rows(rows: torch.Tensor):
    """fp32 rows [N, E] -> (q int16 [N, E] = clamp(rint(v * 2^14), -32767, 32767), norm2 int32 [N] = sum q^2)
    (aaclip_coreset_rows)"""
    r = _f32c(rows)
    require_gpu(r, "coreset_rows")
    if r.dim() != 2:
        raise ValueError("coreset_rows expects rows of [N, E]")
    N, E = r.shape
    q = torch.empty(N, E, dtype=torch.int16, device=r.device)
    norm2 = torch.empty(N, dtype=torch.int32, device=r.device)
    _lib.check(_lib.load().aaclip_coreset_rows(r.data_ptr(), N, E, q.data_ptr(), norm2.data_ptr(), _stream(r.device)),
               "coreset_rows")
    return q, norm2


def coreset_unit_rows(rows: torch.Tensor) -> torch.Tensor:
    """fp32 rows [N, E] -> rows / max(|row|, 1e-12) (aaclip_coreset_unit_rows)"""
    r = _f32c(rows)
    require_gpu(r, "coreset_unit_rows")
    if r.dim() != 2:
        raise ValueError("coreset_unit_rows expects rows of [N, E]")
    out = torch.empty_like(r)
    _lib.check(_lib.load().aaclip_coreset_unit_rows(r.data_ptr(), r.shape[0], r.shape[1], out.data_ptr(), _stream(r.device)),
               "coreset_unit_rows")
    return out


def coreset_select(q: torch.Tensor, norm2: torch.Tensor, n: int, start: int = 0):
    """Greedy k-center selection of n of the N quantised rows, from row `start` (aaclip_coreset_select) ->
    (picks int32 [n], radius2 [n + 1], min_d2 [N]), device tensors; radius2 and min_d2 hold uint32 values in int32
    storage (view the host copies as numpy uint32).  Raises ValueError when a norm2 is 2^29 or more: the dot products would leave int32."""
    require_gpu(q, "coreset_select")
    require_gpu(norm2, "coreset_select")
    if q.dim() != 2 or q.dtype != torch.int16 or norm2.dtype != torch.int32 or norm2.shape != (q.shape[0],) or \
            norm2.device != q.device:
        raise ValueError("coreset_select takes q int16 [N, E] and norm2 int32 [N] of coreset_rows on one device")
    q, norm2 = q.contiguous(), norm2.contiguous()
    N, E = q.shape
    if N and (int(norm2.max()) >= CORESET_NORM2_LIMIT or int(norm2.min()) < 0):
        raise ValueError("coreset_select: a row's norm2 is 2^29 or more (a norm above 1.41); the rows must be unit rows")
    lib = _lib.load()
    dev = q.device
    n, start = int(n), int(start)
    picks = torch.empty(max(n, 0), dtype=torch.int32, device=dev)
    radius2 = torch.empty(max(n, 0) + 1, dtype=torch.int32, device=dev)
    min_d2 = torch.empty(N, dtype=torch.int32, device=dev)
    ws = Workspace.get(dev, max(256, lib.aaclip_coreset_select_workspace_bytes(N, E, n)))
    _lib.check(lib.aaclip_coreset_select(q.data_ptr(), norm2.data_ptr(), N, E, n, start, picks.data_ptr(), radius2.data_ptr(),
                                         min_d2.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)), "coreset_select")
    return picks, radius2, min_d2


def coreset_projection(E: int, dim: int, seed: int = 0) -> torch.Tensor:
    """the seeded Gaussian projection of support_bank_coreset as the GEMM's weight [dim, E] (host tensor)"""
    from . import synth
    return synth.randn("support.coreset.projection", (E, dim), dim ** -0.5, seed).t().contiguous()


def coreset_projected_rows(rows: torch.Tensor, dim: int, seed: int = 0) -> torch.Tensor:
    """fp32 unit rows [N, E] -> unit rows [N, dim]: the library's fp32 GEMM with the seeded projection, then
    coreset_unit_rows.  dim must be a multiple of 128 (the GEMM's column tile)."""
    r = _f32c(rows)
    require_gpu(r, "coreset_projected_rows")
    N, E = r.shape
    if dim % 128 or dim < 128 or dim > 1024:
        raise ValueError("support_bank_coreset: dim must be 0 or a multiple of 128 up to 1024")
    w = coreset_projection(E, dim, seed).to(r.device)
    out = torch.empty(N, dim, dtype=torch.float32, device=r.device)
    gemm(_lib.F32, _lib.EPI_ACT_F32, r, w, None, out)
    return coreset_unit_rows(out)


def support_bank_coreset(seg_tokens_per_image_batch, form, ratio: float, dim: int = 128, seed: int = 0) -> CoresetBank:
    """support_bank's input and concatenation order; per level the rows are (for 0 < dim < E) projected to `dim`
    dimensions and re-normalised, quantised, and n = max(1, ceil(ratio * N)) of them are selected greedily from row 0
    (coreset_select), truncated where the covering radius reaches 0 (every further row duplicates a pick).  The ORIGINAL
    fp32 rows of the picks form the bank that support_nearest and support_map take."""
    import math
    import numpy as np
    if not 0.0 < float(ratio) <= 1.0:
        raise ValueError("support_bank_coreset: ratio must lie in (0, 1]")
    dim = int(dim)
    if dim < 0:
        raise ValueError("support_bank_coreset: dim must not be negative")
    form = support_form(form)
    batches = list(seg_tokens_per_image_batch)
    if not batches:
        raise ValueError("support_bank: no images")
    if torch.is_tensor(batches[0]):
        batches = [batches]
    levels = len(batches[0])
    if levels < 1 or any(len(b) != levels for b in batches):
        raise ValueError("support_bank: every batch must hold the same tap levels")
    require_gpu(batches[0][0], "support_bank_coreset")
    P, E = batches[0][0].shape[1:]
    shots = sum(int(b[0].shape[0]) for b in batches)
    N = shots * P
    n = max(1, min(N, int(math.ceil(float(ratio) * N))))
    used = dim if 0 < dim < E else 0
    rows, index, radii = [], [], []
    for l in range(levels):
        parts = [_f32c(b[l]) for b in batches]
        if any(p.dim() != 3 or tuple(p.shape[1:]) != (P, E) for p in parts):
            raise ValueError("support_bank: seg tokens must be [b, P, E] with one P and E")
        full = torch.cat(parts, dim=0).reshape(N, E)
        q, norm2 = coreset_rows(coreset_projected_rows(full, used, seed) if used else full)
        picks, radius2, _ = coreset_select(q, norm2, n, 0)
        r2 = radius2.cpu().numpy().view(np.uint32)
        zero = np.flatnonzero(r2 == 0)
        kept = int(zero[0]) if zero.size else n
        picks, r2 = picks[:kept].contiguous(), r2[:kept + 1].copy()
        rows.append(support_bank_rows(torch.index_select(full, 0, picks.long()), form))
        index.append(picks)
        radii.append(r2)
    return CoresetBank(rows, form, int(P), shots, index, radii, used)


# ------------------------------------------------------------------------------- tiled inference (csrc/tiles.hip)
def tile_canvas(S: int, G: int, O: int) -> int:
    """The canvas side C = S + (G - 1) * (S - O) of G x G tiles of side S that overlap by O pixels (aaclip_tile_canvas);
    ValueError for S < 1, G < 1, O outside 0 .. S // 2 or a side beyond int."""
    c = _lib.load().aaclip_tile_canvas(int(S), int(G), int(O))
    if c < 0:
        raise ValueError(f"tile_canvas: tile {S}, grid {G}, overlap {O}: tile >= 1, grid >= 1 and 0 <= overlap <= tile // 2")
    return int(c)


def _tile_tensor(t: torch.Tensor, what: str) -> None:
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError(f"{what}: expects a tensor on the GPU (there is no CPU fallback)")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: expects fp32, got {t.dtype}")
    if t.dim() not in (3, 4):
        raise ValueError(f"{what}: expects [n, channels, side, side] or [n, side, side], got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: expects a contiguous tensor")


def _tile_plan(images: int, channels: int, S: int, G: int, O: int, dev: torch.device) -> TilePlan:
    plan = TilePlan()
    plan.images, plan.channels, plan.tile, plan.grid, plan.overlap = images, channels, S, G, O
    plan.stream = _stream(dev)
    return plan


def tile_gather(canvas: torch.Tensor, S: int, G: int, O: int) -> torch.Tensor:
    """canvas fp32 [B, ch, C, C] (or [B, C, C]), C = tile_canvas(S, G, O) -> tiles [B * G * G, ch, S, S] (or
    [B * G * G, S, S]): tile b * G * G + i * G + j is canvas[b, :, i * T : i * T + S, j * T : j * T + S], T = S - O, the
    same bits (aaclip_tile_gather, one launch on the current stream)."""
    S, G, O = int(S), int(G), int(O)
    C_ = tile_canvas(S, G, O)
    _tile_tensor(canvas, "tile_gather")
    if tuple(canvas.shape[-2:]) != (C_, C_):
        raise ValueError(f"tile_gather: tile {S}, grid {G}, overlap {O} need a canvas of side {C_}, got {tuple(canvas.shape)}")
    B = int(canvas.shape[0])
    lead = tuple(canvas.shape[1:-2])
    ch = int(lead[0]) if lead else 1
    tiles = torch.empty((B * G * G,) + lead + (S, S), dtype=torch.float32, device=canvas.device)
    plan = _tile_plan(B, ch, S, G, O, canvas.device)
    _lib.check(_lib.load().aaclip_tile_gather(C.byref(plan), canvas.data_ptr(), tiles.data_ptr()), "tile_gather")
    return tiles


def tile_stitch(tiles: torch.Tensor, G: int, O: int, images: int) -> torch.Tensor:
    """tiles fp32 [images * G * G, ch, S, S] (or [images * G * G, S, S]) -> canvas [images, ch, C, C] (or
    [images, C, C]): a pixel under one tile takes that tile's bits, any other the weighted mean of its 2 or 4 tiles with
    the weights min(y + 1, S - y) * min(x + 1, S - x), in ascending tile order in fp32 (aaclip_tile_stitch, one launch on
    the current stream; forward_utils.tile_stitch_host is the definition)."""
    G, O, images = int(G), int(O), int(images)
    _tile_tensor(tiles, "tile_stitch")
    S = int(tiles.shape[-1])
    C_ = tile_canvas(S, G, O)
    if tiles.shape[-2] != S or images < 0 or tiles.shape[0] != images * G * G:
        raise ValueError(f"tile_stitch: {images} images on a grid of {G} need [{images * G * G}, ..., S, S] tiles, got "
                         f"{tuple(tiles.shape)}")
    lead = tuple(tiles.shape[1:-2])
    ch = int(lead[0]) if lead else 1
    canvas = torch.empty((images,) + lead + (C_, C_), dtype=torch.float32, device=tiles.device)
    plan = _tile_plan(images, ch, S, G, O, tiles.device)
    _lib.check(_lib.load().aaclip_tile_stitch(C.byref(plan), tiles.data_ptr(), canvas.data_ptr()), "tile_stitch")
    return canvas


# ------------------------------------------------------------------------------- heat-map overlays (csrc/overlay.hip)
OVERLAY_PANELS = ("frame", "heat", "truth")           # the order of the panels in the output; bit i selects panel i
OVERLAY_LUTS = ("jet", "gray")
OVERLAY_MAX_THICKNESS = 8
_OVERLAY_LUTS: Dict[tuple, torch.Tensor] = {}


def overlay_lut(name: str) -> torch.Tensor:
    """The colour table `name` as a host uint8 [256, 3] tensor (RGB), defined in integers so that no rounding tie occurs:
    "jet": lut[i][ch] = clamp(383 - |4 * i - 255 * c|, 0, 255), c = 3, 2, 1 for R, G, B -- the classic
    clamp(1.5 - |4 v - c|) ramp at v = i / 255, rounded half up; "gray": lut[i] = (i, i, i).  Neither is claimed to equal
    another library's bytes.  ValueError for any other name."""
    if name == "jet":
        i = torch.arange(256, dtype=torch.int64).view(256, 1)
        c = torch.tensor([3, 2, 1], dtype=torch.int64).view(1, 3)
        return (383 - (4 * i - 255 * c).abs()).clamp(0, 255).to(torch.uint8)
    if name == "gray":
        return torch.arange(256, dtype=torch.uint8).view(256, 1).repeat(1, 3)
    raise ValueError(f"overlay_lut: unknown colour table {name!r} (one of {', '.join(OVERLAY_LUTS)})")


def overlay_panels(panels, has_truth: bool) -> Tuple[str, ...]:
    """The panels of a call in output order: None is all three, without "truth" when there is no truth mask; ValueError
    for an empty selection, an unknown or repeated name, or "truth" without a truth mask."""
    if panels is None:
        return OVERLAY_PANELS if has_truth else OVERLAY_PANELS[:2]
    panels = (panels,) if isinstance(panels, str) else tuple(panels)
    if not panels or any(p not in OVERLAY_PANELS for p in panels) or len(set(panels)) != len(panels):
        raise ValueError(f"overlay: panels must be a non-empty subset of {OVERLAY_PANELS}, got {panels}")
    if "truth" in panels and not has_truth:
        raise ValueError("overlay: the truth panel needs a truth mask")
    return tuple(p for p in OVERLAY_PANELS if p in panels)


def _overlay_colour(v, what: str) -> Tuple[int, int, int]:
    v = tuple(int(c) for c in v)
    if len(v) != 3 or any(not 0 <= c <= 255 for c in v):
        raise ValueError(f"overlay_render: {what} must be an RGB triple of bytes, got {v}")
    return v


def overlay_render(frames: torch.Tensor, maps: torch.Tensor, range_record: Optional[torch.Tensor] = None,
                   pred: Optional[torch.Tensor] = None, truth: Optional[torch.Tensor] = None, alpha: float = 0.5,
                   lut="jet", thickness: int = 1, panels=None, pred_colour=(255, 255, 255), truth_colour=(0, 255, 0),
                   mean=CLIP_MEAN, std=CLIP_STD) -> torch.Tensor:
    """frames fp32 [B, 3, H, W] (the normalised model input), maps fp32 [B, H, W] (raw scores), range_record the record
    of metrics_range or None, pred / truth uint8 [B, H, W] or None -> uint8 [B, n * H, W, 3]: the n panels of `panels`
    (a non-empty subset of ("frame", "heat", "truth"), always in that order) stacked vertically; the default is all
    three, without "truth" when truth is None.  alpha256 = round(alpha * 256) is the frame's weight in a blend; lut a
    table name (overlay_lut) or a uint8 [256, 3] device tensor; thickness T in 0 .. 8 the reach of the mask contours.
    One launch on the current stream (aaclip_overlay_render; forward_utils.render_overlays_host is the definition, byte
    for byte).  ValueError for host tensors, wrong dtypes or shapes, non-contiguous inputs and an unknown table."""
    what = "overlay_render"
    for t, name, dtype, dims in ((frames, "frames", torch.float32, 4), (maps, "maps", torch.float32, 3),
                                 (pred, "pred", torch.uint8, 3), (truth, "truth", torch.uint8, 3)):
        if t is None and name in ("pred", "truth"):
            continue
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError(f"{what}: {name} must be a tensor on the GPU (there is no CPU fallback)")
        if t.dtype != dtype or t.dim() != dims:
            raise ValueError(f"{what}: {name} must be {dtype} with {dims} dimensions, got {t.dtype} {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be contiguous")
        if t.device != frames.device:
            raise ValueError(f"{what}: {name} is on another device than frames")
    B, ch, H, W = (int(v) for v in frames.shape)
    if ch != 3 or H < 1 or W < 1:
        raise ValueError(f"{what}: frames must be [B, 3, H, W] with H, W >= 1, got {tuple(frames.shape)}")
    for t, name in ((maps, "maps"), (pred, "pred"), (truth, "truth")):
        if t is not None and tuple(t.shape) != (B, H, W):
            raise ValueError(f"{what}: {name} must be [{B}, {H}, {W}] like frames, got {tuple(t.shape)}")
    dev = frames.device
    if range_record is not None and (not torch.is_tensor(range_record) or not range_record.is_cuda
                                     or range_record.dtype != torch.int64 or range_record.numel() != 3
                                     or not range_record.is_contiguous() or range_record.device != dev):
        raise ValueError(f"{what}: range_record must be the device record of metrics_range (int64 [3]) or None")
    panels = overlay_panels(panels, truth is not None)
    bits = sum(1 << OVERLAY_PANELS.index(p) for p in panels)
    alpha256 = int(round(float(alpha) * 256))
    if not 0 <= alpha256 <= 256:
        raise ValueError(f"{what}: alpha must be in 0 .. 1, got {alpha}")
    thickness = int(thickness)
    if not 0 <= thickness <= OVERLAY_MAX_THICKNESS:
        raise ValueError(f"{what}: thickness must be in 0 .. {OVERLAY_MAX_THICKNESS}, got {thickness}")
    pred_colour, truth_colour = _overlay_colour(pred_colour, "pred_colour"), _overlay_colour(truth_colour, "truth_colour")
    mean, std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
    if len(mean) != 3 or len(std) != 3 or any(not 0.0 < v < float("inf") for v in std):
        raise ValueError(f"{what}: mean and std must have three entries, std positive and finite")
    if isinstance(lut, str):
        table = _OVERLAY_LUTS.get((dev, lut))
        if table is None:
            table = _OVERLAY_LUTS[(dev, lut)] = overlay_lut(lut).to(dev)
    else:
        table = lut
        if (not torch.is_tensor(table) or not table.is_cuda or table.dtype != torch.uint8 or tuple(table.shape) != (256, 3)
                or not table.is_contiguous() or table.device != dev):
            raise ValueError(f"{what}: lut must be a table name or a contiguous uint8 [256, 3] tensor on the frames' device")
    plan = OverlayPlan()
    plan.images, plan.height, plan.width, plan.panels = B, H, W, bits
    plan.alpha256, plan.thickness = alpha256, thickness
    for c in range(3):
        plan.pred_colour[c], plan.truth_colour[c] = pred_colour[c], truth_colour[c]
        plan.mean[c], plan.std[c] = mean[c], std[c]
    plan.stream = _stream(dev)
    out = torch.empty((B, len(panels) * H, W, 3), dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().aaclip_overlay_render(C.byref(plan), frames.data_ptr(), maps.data_ptr(), _ptr(range_record),
                                                 _ptr(pred), _ptr(truth), table.data_ptr(), out.data_ptr()), what)
    return out


# ------------------------------------------------------------------------------- PNG encoding (csrc/png.hip)
PNG_SEGMENT_BYTES = 32768       # csrc/png_plan.h


def png_segments(H: int, W: int, C: int) -> Dict[str, int]:
    """The geometry of an H x W x C image's filtered stream (csrc/png_plan.h): row_bytes = 1 + W * C, rows_per_segment =
    max(1, 32768 // row_bytes), segments per image, stream_bytes = H * row_bytes and capacity = 8 + stream_bytes +
    5 * segments, the largest zlib stream of one image.  ValueError for C outside {1, 3}, negative sizes and a row of
    more than 32768 bytes."""
    H, W, C = int(H), int(W), int(C)
    if C not in (1, 3) or H < 0 or W < 0:
        raise ValueError(f"png_segments: H and W must not be negative and C must be 1 or 3, got {H} x {W} x {C}")
    row = 1 + W * C
    if row > PNG_SEGMENT_BYTES:
        raise ValueError(f"png_segments: a filtered row of {row} bytes exceeds {PNG_SEGMENT_BYTES}")
    rps = max(1, PNG_SEGMENT_BYTES // row)
    segs = -(-H // rps)
    return {"row_bytes": row, "rows_per_segment": rps, "segments": segs, "stream_bytes": H * row,
            "capacity": 8 + H * row + 5 * segs}


def png_encode(pixels: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """pixels uint8 [images, H, W, C] with C in {1, 3}, or [images, H, W] for C = 1, contiguous, on the GPU, at any
    byte offset of its storage -> (payload uint8 [capacity], offsets int64 [images + 1]), both on the device: image i's
    zlib stream (the content of its PNG's IDAT chunk) is payload[offsets[i]:offsets[i + 1]]; forward_utils.png_files
    wraps the streams into files.  Two launches on the current stream (aaclip_png_encode; forward_utils.png_encode_host
    is the definition, byte for byte).  ValueError for a host tensor, a wrong dtype or shape and a non-contiguous
    input."""
    what = "png_encode"
    if not torch.is_tensor(pixels) or not pixels.is_cuda:
        raise ValueError(f"{what}: pixels must be a tensor on the GPU (there is no CPU fallback)")
    if pixels.dtype != torch.uint8 or pixels.dim() not in (3, 4):
        raise ValueError(f"{what}: pixels must be uint8 [images, H, W, C] or [images, H, W], got {pixels.dtype} "
                         f"{tuple(pixels.shape)}")
    if not pixels.is_contiguous():
        raise ValueError(f"{what}: pixels must be contiguous")
    images, H, W = (int(v) for v in pixels.shape[:3])
    ch = int(pixels.shape[3]) if pixels.dim() == 4 else 1
    if ch not in (1, 3):
        raise ValueError(f"{what}: pixels must have 1 or 3 channels, got {ch}")
    dev = pixels.device
    plan = _lib.PngPlan()
    plan.images, plan.height, plan.width, plan.channels = images, H, W, ch
    plan.stream = _stream(dev)
    lib = _lib.load()
    offsets = torch.zeros(images + 1, dtype=torch.int64, device=dev)
    if images == 0:
        return torch.empty(0, dtype=torch.uint8, device=dev), offsets
    capacity, ws_bytes = lib.aaclip_png_capacity_bytes(C.byref(plan)), lib.aaclip_png_workspace_bytes(C.byref(plan))
    if capacity == 0:
        png_segments(H, W, ch)
        raise ValueError(f"{what}: the library refuses {images} images of {H} x {W} x {ch}")
    payload = torch.empty(capacity, dtype=torch.uint8, device=dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.aaclip_png_encode(C.byref(plan), pixels.data_ptr(), ws.data_ptr(), ws_bytes, payload.data_ptr(), capacity,
                                     offsets.data_ptr()), what)
    return payload, offsets


# ------------------------------------------------------------------------------- fused optimizer step (csrc/optim.hip)
OPTIM_RECORD_FLOATS = 2         # fp32 words of aaclip_optim_record: total_norm, clip_coef
OPTIM_MAX_GROUPS = _lib.OPTIM_MAX_GROUPS


def _optim_tensor(t: torch.Tensor, what: str, like: Optional[torch.Tensor] = None) -> None:
    """the optimizer kernels take fp32, contiguous tensors on one GPU as they are: nothing is cast or copied"""
    if not torch.is_tensor(t):
        raise TypeError(f"{what}: expected a tensor, got {type(t).__name__}")
    require_gpu(t, what)
    if t.dtype != torch.float32:
        raise TypeError(f"{what}: {t.dtype} tensor; parameters, gradients and optimizer state are fp32 in this library")
    if t.is_sparse or t.layout != torch.strided or not t.is_contiguous():
        raise ValueError(f"{what}: the tensor must be dense and contiguous")
    if like is not None and (t.shape != like.shape or t.device != like.device):
        raise ValueError(f"{what}: shape {tuple(t.shape)} on {t.device} does not match its parameter's "
                         f"{tuple(like.shape)} on {like.device}")


class OptimPack:
    """A tensor list in the form the library reads (struct aaclip_optim_tensors), checked once and reusable from step to
    step: params / grads / exp_avgs / exp_avg_sqs (equally long lists of fp32, contiguous tensors on one GPU; all but
    grads may be None for a list that only optim_grad_norm reads) and group_of (index into the groups of
    optim_adam_step per tensor).  set_grad(i, g) swaps one gradient without rebuilding the list."""

    def __init__(self, params, grads, exp_avgs=None, exp_avg_sqs=None, group_of=None, what="optim"):
        grads = list(grads)
        full = params is not None
        if full:
            params, exp_avgs, exp_avg_sqs, group_of = list(params), list(exp_avgs), list(exp_avg_sqs), list(group_of)
            if not (len(params) == len(grads) == len(exp_avgs) == len(exp_avg_sqs) == len(group_of)):
                raise ValueError(f"{what}: params, grads, exp_avgs, exp_avg_sqs and group_of must be equally long")
            for p, g, m, v in zip(params, grads, exp_avgs, exp_avg_sqs):
                _optim_tensor(p, what)
                for t in (g, m, v):
                    _optim_tensor(t, what, like=p)
        else:
            for g in grads:
                _optim_tensor(g, what)
        self.params, self.grads, self.exp_avgs, self.exp_avg_sqs = params, grads, exp_avgs, exp_avg_sqs
        self.group_of = [int(k) for k in group_of] if full else [0] * len(grads)
        self.device = grads[0].device if grads else None
        if any(g.device != self.device for g in grads):
            raise ValueError(f"{what}: the tensors must be on one device")
        if full:
            rows = [(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), k)
                    for p, g, m, v, k in zip(params, grads, exp_avgs, exp_avg_sqs, self.group_of)]
        else:
            rows = [(None, g.data_ptr(), None, None, g.numel(), 0) for g in grads]
        self.items = (_lib.OptimTensor * max(len(rows), 1))(*rows)
        self.struct = _lib.OptimTensors(items=self.items, count=len(rows))
        self.norm_workspace_bytes = int(_lib.load().aaclip_optim_grad_norm_workspace_bytes(C.byref(self.struct)))

    def __len__(self):
        return len(self.grads)

    def set_grad(self, i: int, g: torch.Tensor) -> None:
        """the caller has checked g (fp32, contiguous, the parameter's shape and device)"""
        self.grads[i] = g
        self.items[i].g = g.data_ptr()


def _optim_record_ok(record: torch.Tensor, dev) -> bool:
    return (record.dtype == torch.float32 and record.numel() == OPTIM_RECORD_FLOATS and record.is_contiguous()
            and (dev is None or record.device == dev))


def optim_grad_norm(grads, max_norm: float, record: Optional[torch.Tensor] = None,
                    workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> record, fp32 [2] on the device: the 2-norm over all of `grads` (a list of tensors, or an OptimPack) and
    clip_coef = min(1, max_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_'s formula).  Per-chunk fp64 sums in
    workspace slots, one workgroup adds them: no atomics, the same inputs give the same bits.  The gradients are only
    read, nothing comes back to the host.  record / workspace: buffers to reuse (fp32 [2]; uint8 of at least
    pack.norm_workspace_bytes bytes); allocated when None."""
    pack = grads if isinstance(grads, OptimPack) else OptimPack(None, grads, what="optim_grad_norm")
    if not float(max_norm) > 0.0:
        raise ValueError(f"optim_grad_norm: max_norm must be above 0, got {max_norm}")
    if pack.device is None and record is None:
        raise ValueError("optim_grad_norm: no gradients and no record to tell the device from")
    dev = pack.device if pack.device is not None else record.device
    need = pack.norm_workspace_bytes
    if record is None:
        record = torch.empty(OPTIM_RECORD_FLOATS, dtype=torch.float32, device=dev)
    elif not _optim_record_ok(record, dev):
        raise ValueError("optim_grad_norm: record must be a contiguous fp32 [2] tensor on the gradients' device")
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    elif workspace.dtype != torch.uint8 or workspace.device != dev or workspace.numel() < need:
        raise ValueError(f"optim_grad_norm: workspace must be a uint8 tensor of at least {need} bytes on {dev}")
    _lib.check(_lib.load().aaclip_optim_grad_norm(C.byref(pack.struct), float(max_norm), record.data_ptr(),
                                                  workspace.data_ptr(), workspace.numel(), _stream(dev)),
               "optim_grad_norm")
    return record


def optim_adam_step(params, grads=None, exp_avgs=None, exp_avg_sqs=None, group_of=None, groups=(),
                    record: Optional[torch.Tensor] = None) -> None:
    """One Adam / AdamW step of every tensor in place, in as few launches as the list needs (24 tensors and 640 chunks of
    16384 elements per launch).  params .. group_of: lists (group_of[i]: index into `groups` of tensor i), or an
    OptimPack in place of params.  groups: up to OPTIM_MAX_GROUPS dicts {"lr", "beta1", "beta2", "eps", "weight_decay",
    "decoupled" (True: AdamW), "step" (the step being taken, >= 1)}.  record: the device record of optim_grad_norm,
    whose clip_coef scales every gradient as it is read (the gradients in memory stay as they are); None: no clipping.
    Arithmetic: include/aaclip.h aaclip_optim_adam_step."""
    groups = list(groups)
    if not 1 <= len(groups) <= OPTIM_MAX_GROUPS:
        raise ValueError(f"optim_adam_step: 1 .. {OPTIM_MAX_GROUPS} groups per call, got {len(groups)}")
    pack = params if isinstance(params, OptimPack) else OptimPack(params, grads, exp_avgs, exp_avg_sqs, group_of,
                                                                  "optim_adam_step")
    if pack.params is None:
        raise ValueError("optim_adam_step: the pack holds gradients only")
    if any(not 0 <= k < len(groups) for k in pack.group_of):
        raise ValueError(f"optim_adam_step: a group index lies outside the {len(groups)} groups")
    if not len(pack):
        return
    if record is not None and not _optim_record_ok(record, pack.device):
        raise ValueError("optim_adam_step: record must be the fp32 [2] record of optim_grad_norm on the parameters' device")
    cg = (_lib.OptimGroup * len(groups))(*[
        (float(h["lr"]), float(h["beta1"]), float(h["beta2"]), float(h["eps"]), float(h["weight_decay"]),
         1 if h["decoupled"] else 0, int(h["step"])) for h in groups])
    _lib.check(_lib.load().aaclip_optim_adam_step(C.byref(pack.struct), cg, len(groups), _ptr(record),
                                                  _stream(pack.device)), "optim_adam_step")
