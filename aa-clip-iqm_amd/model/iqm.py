"""IQM side branch on the MI355X path: the "Improved Querying" transformer of reference
model/iqm.py (IQM, IQMEncoder, IQMLayer, IQM_Attention ...) and the glue around it in AdaptedCLIP.forward
(reference model/adapter.py:186-269), eval mode.

Two queries per image (normal / abnormal), started from an MLP of the CLS row plus a sinusoidal position, run through
`num_hidden_layers` layers of {self-attention, cross-attention to the projected patch rows of the four tap levels,
cross-attention to the projected anchors, fixed 0.4/0.3/0.3 fusion, GELU feed-forward}, then a LayerNorm.

Parameters carry the reference's names, so `state_dict()` of AdaptedCLIP matches the reference key for key
(`iqm.encoder.layer.0.crossattention.attention.key.weight`, `class_query_mlp.2.bias`, `query_adapters.1.fc.weight`,
`iqm_layer_norm.weight`, `pos_embedding` ...).  Two deliberate differences, both because the reference's behaviour
cannot be reproduced or checkpointed:
  * `visual_feature_proj` / `text_feature_proj` are created by the reference INSIDE forward with fresh random weights
    (adapter.py:213-218, 241-243) and never saved; here they are ordinary parameters (Linear(hidden, hidden) and
    Linear(2, 768): 2 because the anchors arrive as [B, 768, 2]) that are initialised once and saved with the rest;
  * dropout is the identity.
There is ONE forward: the training path (aaclip_hip.autograd.iqm_queries) runs this same code with a `record` dict that
collects what its backward needs (IQM.forward lists the keys), so inference and training cannot drift apart -- in the
projected form and in the folded 16-bit form of the visual cross-attention alike.
The modules below are parameter containers: every product runs on the library's MFMA GEMM, the rest on the small
kernels of csrc/iqm.hip (aaclip_small_attention, aaclip_residual_layernorm, ...).
"""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch import nn

from aaclip_hip import engine
from aaclip_hip._lib import EPI_ACT_F32, EPI_BIAS, EPI_BIAS_GELU


def linear_f32(code: int, x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, act: int = 0,
               transpose: bool = False) -> torch.Tensor:
    """fp32 output of a Linear on the GEMM: act(x W^T + bias) for x [M, in] in the compute dtype and the Linear's own
    weight [out, in] (prepared once, engine.CACHE); transpose: x [M, out] -> x W, the product on the transposed weight."""
    w = engine.CACHE.get(weight, code, "transpose") if transpose else engine.CACHE.get(weight, code)
    out = torch.empty(x.shape[0], w.shape[0], dtype=torch.float32, device=x.device)
    return engine.gemm(code, EPI_ACT_F32, x, w, None if bias is None else engine._f32c(bias), out, act=act)


class IQMOutput:
    """What the reference returns as iqm_outputs (a transformers BaseModelOutputWithPoolingAndCrossAttentions):
    callers read .last_hidden_state [B, 2, hidden] (test_last.py:104) and .pooler_output."""

    def __init__(self, last_hidden_state: torch.Tensor, pooler_output: Optional[torch.Tensor] = None):
        self.last_hidden_state = last_hidden_state
        # reference model/iqm.py:659-660: row 0 of the ENCODER output.  AdaptedCLIP later replaces last_hidden_state by
        # its LayerNorm (reference model/adapter.py:265) and leaves pooler_output as it was, i.e. pre-LayerNorm.
        self.pooler_output = last_hidden_state[:, 0, :] if pooler_output is None else pooler_output


class _SelfOutput(nn.Module):          # reference model/iqm.py:143-154 / :219-230
    def __init__(self, d_in: int, d: int, eps: float):
        super().__init__()
        self.dense = nn.Linear(d_in, d)
        self.LayerNorm = nn.LayerNorm(d, eps=eps)


class _MultiHeadAttention(nn.Module):  # reference model/iqm.py:23-58
    def __init__(self, d: int, d_kv: int):
        super().__init__()
        self.query = nn.Linear(d, d)
        self.key = nn.Linear(d_kv, d)
        self.value = nn.Linear(d_kv, d)


class _Attention(nn.Module):           # reference model/iqm.py:157-162
    def __init__(self, d: int, d_kv: int, eps: float):
        super().__init__()
        self.attention = _MultiHeadAttention(d, d_kv)
        self.output = _SelfOutput(d, d, eps)


class _Intermediate(nn.Module):        # reference model/iqm.py:206-217
    def __init__(self, d: int, inter: int):
        super().__init__()
        self.dense = nn.Linear(d, inter)


class IQMLayer(nn.Module):             # reference model/iqm.py:234-259
    def __init__(self, d: int, d_enc: int, d_txt: int, inter: int, eps: float):
        super().__init__()
        self.attention = _Attention(d, d, eps)
        self.crossattention = _Attention(d, d_enc, eps)
        self.text_crossattention = _Attention(d, d_txt, eps)
        self.intermediate = _Intermediate(d, inter)          # the non-query feed-forward: parameters only (the path
        self.output = _SelfOutput(inter, d, eps)             # never has more than query_length tokens, iqm.py:323)
        self.intermediate_query = _Intermediate(d, inter)
        self.output_query = _SelfOutput(inter, d, eps)


class _Encoder(nn.Module):
    def __init__(self, layers: int, d: int, d_enc: int, d_txt: int, inter: int, eps: float):
        super().__init__()
        self.layer = nn.ModuleList([IQMLayer(d, d_enc, d_txt, inter, eps) for _ in range(layers)])


class IQM(nn.Module):
    """reference model/iqm.py:497-673 (IQMConfig defaults :453-494: intermediate 2048, gelu, eps 1e-12,
    cross_attention_frequency 1)."""

    def __init__(self, hidden_size: int = 768, num_hidden_layers: int = 2, num_attention_heads: int = 8,
                 encoder_hidden_size: int = 768, text_encoder_hidden_size: int = 768, intermediate_size: int = 2048,
                 layer_norm_eps: float = 1e-12):
        super().__init__()
        if hidden_size % num_attention_heads:
            raise ValueError("The hidden size (%d) is not a multiple of the number of attention heads (%d)"
                             % (hidden_size, num_attention_heads))
        self.hidden_size, self.num_attention_heads, self.eps = hidden_size, num_attention_heads, layer_norm_eps
        self.layernorm = nn.LayerNorm(hidden_size, eps=layer_norm_eps)
        self.encoder = _Encoder(num_hidden_layers, hidden_size, encoder_hidden_size, text_encoder_hidden_size,
                                intermediate_size, layer_norm_eps)

    def cross_rows_form(self, nq: int, width: int) -> bool:
        """Whether a cross-attention of nq queries per image over rows `width` wide takes the aaclip_cross_rows form of
        _attend: queries x heads in {4, 8, 12, 16} and a row width of that kernel (and of aaclip_cross_rows_backward,
        so these are also the configurations the training path covers)."""
        R = nq * self.num_attention_heads
        return R % 4 == 0 and R <= 16 and width in (256, 512, 768, 1024)

    def levels_form_has_backward(self, nq: int, levels: dict) -> bool:
        """Whether a record of the folded form (encoder_levels) has a backward: the domain of
        aaclip_cross_rows_levels_backward -- queries x heads in {4, 8, 12, 16}, rows 768 or 1024 wide, 1..4 levels."""
        R = nq * self.num_attention_heads
        return R % 4 == 0 and R <= 16 and levels["width"] in (768, 1024) and 1 <= len(levels["rows"]) <= 4

    def _tail(self, att: _Attention, h: torch.Tensor, code: int, ebar=None, ctx=None, record=None, key: str = ""):
        """The end of one IQM_Attention: ctx [B*nq, D] as it is, or the value product of the probability-weighted rows
        ebar [B*nq*H, Dk] and its head-diagonal blocks; then output.dense and LayerNorm(. + h)."""
        dt = engine.torch_dtype(code)
        if ctx is None:
            ctx = engine.head_diag(linear_f32(code, ebar.to(dt), att.attention.value.weight, att.attention.value.bias),
                                   self.num_attention_heads)
        dense = linear_f32(code, ctx.to(dt), att.output.dense.weight, att.output.dense.bias)
        if record is not None:
            record[key + "ctx"], record[key + "dense"] = ctx, dense
            if ebar is not None:
                record[key + "ebar"] = ebar
        return engine.residual_layernorm(dense, h, att.output.LayerNorm, self.eps)

    # ---- one IQM_Attention: q from h [B*nq, D] (fp32), k/v = Linear(enc) where enc is [B*Lk, Dk] in the compute dtype
    def _attend(self, att: _Attention, h: torch.Tensor, enc: Optional[torch.Tensor], B: int, nq: int, Lk: int,
                code: int, enc_proj=None, enc_levels=None, record=None, key: str = "") -> torch.Tensor:
        """record (see forward) takes this attention's entries under the prefix `key`."""
        dt = engine.torch_dtype(code)
        D, H = self.hidden_size, self.num_attention_heads
        rows_form = enc_levels is None and enc is not None and self.cross_rows_form(nq, enc.shape[-1])
        if record is not None and not rows_form and enc is not None:
            raise NotImplementedError("IQM: a record covers the self-attention, the folded levels and the aaclip_cross_rows "
                                      "form of the cross-attentions (queries x heads in {4, 8, 12, 16}, row widths 256 / "
                                      "512 / 768 / 1024), not the small_attention path")
        hq = h.to(dt)                                      # [B*nq, D]: 2 rows per image
        q = linear_f32(code, hq, att.attention.query.weight, att.attention.query.bias)
        if enc_levels is not None or rows_form:
            qm = engine.head_expand(q, H, 1.0 / math.sqrt(D // H), code)                         # [B*nq*H, D]
            qt = linear_f32(code, qm, att.attention.key.weight, transpose=True)                  # [B*nq*H, Dk]
            if record is not None:
                record[key + "qm"], record[key + "qt"] = qm.float(), qt
        if enc_levels is not None:
            # the rows are level s's LayerNorm'ed tap rows t, enc = P (W_qa[s] t) + b_p (query_adapters, torch.cat,
            # visual_feature_proj: reference model/adapter.py:205-221), every step linear: all of it moves to the query
            # side and behind the weighted sums (include/aaclip.h, aaclip_cross_rows_levels) -- no per-row product at all
            lv = enc_levels
            pw, pb = enc_proj
            qx = linear_f32(code, qt.to(dt), pw, transpose=True)
            nseg, Dk = len(lv["rows"]), lv["width"]
            u = torch.empty(B * nq * H, nseg * Dk, dtype=torch.float32, device=h.device)
            engine.gemm(code, EPI_ACT_F32, qx.to(dt), lv["w_in"], None, u)        # u[., s] = W_qa[s]^T qx
            tbar = engine.cross_rows_levels(u, lv["rows"], B, nq * H, lv["rows_per_image"], lv["row0"], lv["keys"], Dk)
            xbar = torch.empty(B * nq * H, pw.shape[1], dtype=torch.float32, device=h.device)
            engine.gemm(code, EPI_ACT_F32, tbar.to(dt), lv["w_out"], None, xbar)  # sum_s W_qa[s] tbar[., s]
            if record is not None:
                record.update({key + "qx": qx, key + "u": u, key + "tbar": tbar, key + "xbar": xbar})
            return self._tail(att, h, code, ebar=linear_f32(code, xbar.to(dt), pw, pb), record=record, key=key)
        if rows_form:
            # cross-attention over MANY rows for a handful of queries: W_k moves to the query side and W_v behind the
            # probability-weighted sum of the raw rows (include/aaclip.h, aaclip_cross_rows): the reference's key /
            # value projections of all Lk rows (2 x Lk x Dk x D MACs per image, reference model/iqm.py:116-121) become
            # two [nq*H, .] products.  b_k only shifts every score of a row by the same amount: softmax-invariant.
            if enc_proj is not None:
                # the rows are enc = P x + b_p of raw rows x (AdaptedCLIP.visual_feature_proj on the concatenated levels,
                # reference model/adapter.py:213-221): the same algebra once more -- (P^T qt) . x_j + const on the way
                # in, P (sum_j p_j x_j) + b_p on the way out -- and the [B*Lk, .] projection is never computed
                pw, pb = enc_proj
                qx = linear_f32(code, qt.to(dt), pw, transpose=True)
                xbar = engine.cross_rows(qx, enc, B, nq * H, Lk, code)
                ebar = linear_f32(code, xbar.to(dt), pw, pb)
                if record is not None:
                    record[key + "qx"], record[key + "xbar"] = qx, xbar
            elif enc.dtype in (torch.float16, torch.bfloat16) and enc.shape[-1] in (768, 1024):
                # 16-bit rows: the matrix-core kernel, one segment (the anchor tokens of the text cross-attention)
                ebar = engine.cross_rows_levels(qt, [enc], B, nq * H, Lk, 0, Lk, enc.shape[-1])
            else:
                ebar = engine.cross_rows(qt, enc, B, nq * H, Lk, code)                           # [B*nq*H, Dk] fp32
            return self._tail(att, h, code, ebar=ebar, record=record, key=key)
        src = hq if enc is None else enc
        k = torch.empty(src.shape[0], D, dtype=dt, device=h.device)      # compute dtype (fp32 on the fp32 path)
        v = torch.empty_like(k)
        engine.gemm(code, EPI_BIAS, src, engine.CACHE.get(att.attention.key.weight, code),
                    engine._f32c(att.attention.key.bias), k)
        engine.gemm(code, EPI_BIAS, src, engine.CACHE.get(att.attention.value.weight, code),
                    engine._f32c(att.attention.value.bias), v)
        if record is not None:
            record[key + "q"], record[key + "k"], record[key + "v"] = q, k.float(), v.float()
        return self._tail(att, h, code, ctx=engine.small_attention(q, k, v, B, nq, Lk, H, code), record=record, key=key)

    def forward(self, query_embeds: torch.Tensor, query_length: Optional[int] = None,
                encoder_hidden_states: Optional[torch.Tensor] = None,
                text_encoder_hidden_states: Optional[torch.Tensor] = None, code: Optional[int] = None,
                encoder_proj=None, encoder_levels=None, record: Optional[dict] = None, **_unused):
        """query_embeds fp32 [B, nq, D]; encoder_hidden_states [B, Lv, D] and text_encoder_hidden_states [B, Lt, D] in
        the compute dtype (or fp32) -> IQMOutput.  reference model/iqm.py:572-673 with all masks zero.
        encoder_proj = (weight, bias): encoder_hidden_states are the rows BEFORE that Linear; it is folded into the
        cross-attention (see _attend) instead of being applied to every row.
        encoder_levels (instead of encoder_hidden_states; AdaptedCLIP._iqm_levels builds it): the LayerNorm'ed rows of
        the tap levels themselves plus the concatenated query_adapters weights -- the level projections fold too.

        record: None keeps nothing alive.  A dict receives what a backward of this forward needs (the training path,
        aaclip_hip.autograd.IqmQueries, saves its values), and the forward is the same launches plus, per layer, the one
        EPI_ACT_F32 product of the pre-GELU rows.  Every entry is fp32 (16-bit results are stored as fp32 copies)
        except `vis` and `txt`.  The keys, with l the layer index:
          vis, txt               the key / value rows [B*Lv, D] and [B*Lt, Dt] as the cross-attentions read them; with
                                 encoder_levels, vis is that dict itself (its row buffers are what the kernel read)
          last                   the encoder output [B*nq, D]
          {l}.h  .a  .c  .mix    the layer's input, the outputs of the self- and the visual cross-attention, the fusion
          {l}.z  .inter  .dense  the feed-forward: pre-GELU rows, GELU output, output_query.dense
          {l}.a. {l}.c. {l}.t.   prefixes of the self-, the visual cross- and the text cross-attention:
            ctx, dense           all three: the attention output [B*nq, D] and output.dense of it
            q, k, v              the self-attention's projections
            qm, qt, ebar         both cross-attentions: the head-expanded queries, those times W_k, the weighted rows
            qx, xbar             the visual one: qt times encoder_proj's weight, the weighted raw rows
            u, tbar              the visual one with encoder_levels: qx times the query_adapters weights [B*nq*H,
                                 levels*Dk] and the weighted tap rows per level (xbar is then their sum through w_out)
        AdaptedCLIP._iqm_branch adds cls, t1, query and te (the CLS rows, class_query_mlp's hidden rows, query_embeds,
        the anchors).  The self-attention, the aaclip_cross_rows form and the folded levels inside the domain of
        aaclip_cross_rows_levels_backward have a backward: with a record, anything else raises NotImplementedError
        before a launch."""
        if (record is not None and encoder_levels is not None
                and not self.levels_form_has_backward(query_embeds.shape[1], encoder_levels)):
            raise NotImplementedError("IQM: no record (no backward) for these folded levels: "
                                      "aaclip_cross_rows_levels_backward covers queries x heads in {4, 8, 12, 16} over "
                                      "1..4 levels of rows 768 or 1024 wide")
        engine.require_gpu(query_embeds, "IQM")
        if code is None:
            code = engine.dtype_code(getattr(self, "precision", "fp32"))
        # no split-fp16 GEMMs on this side branch: fp32 products under fp16x2 (with encoder_levels the visual
        # cross-attention still reads fp16 key / value rows and fp16 probabilities, see AdaptedCLIP.forward)
        code = engine.plain_code(code)
        dt = engine.torch_dtype(code)
        B, nq, D = query_embeds.shape
        if (encoder_hidden_states is None and encoder_levels is None) or text_encoder_hidden_states is None:
            raise ValueError("encoder_hidden_states must be given for cross-attention layers")     # iqm.py:289
        if encoder_levels is not None:
            if encoder_proj is None or (nq * self.num_attention_heads) > 16:
                raise ValueError("encoder_levels needs encoder_proj and at most 16 queries x heads per image")
            vis, Lv = None, encoder_levels["keys"] * len(encoder_levels["rows"])
        else:
            vis = encoder_hidden_states.to(dt).reshape(-1, encoder_hidden_states.shape[-1]).contiguous()
            Lv = encoder_hidden_states.shape[1]
        txt = text_encoder_hidden_states.to(dt).reshape(-1, text_encoder_hidden_states.shape[-1]).contiguous()
        Lt = text_encoder_hidden_states.shape[1]
        rec = record is not None
        if rec:
            record["vis"], record["txt"] = (encoder_levels if encoder_levels is not None else vis), txt
        h = engine.residual_layernorm(engine._f32c(query_embeds).reshape(B * nq, D), None, self.layernorm, self.eps)
        for l, layer in enumerate(self.encoder.layer):
            a = self._attend(layer.attention, h, None, B, nq, nq, code, record=record, key=f"{l}.a.")
            c = self._attend(layer.crossattention, a, vis, B, nq, Lv, code, enc_proj=encoder_proj,
                             enc_levels=encoder_levels, record=record, key=f"{l}.c.")
            t = self._attend(layer.text_crossattention, c, txt, B, nq, Lt, code, record=record, key=f"{l}.t.")
            mix = engine.combine3(a, c, t, 0.4, 0.3, 0.3)                                            # iqm.py:311-315
            mi, mo = layer.intermediate_query.dense, layer.output_query.dense
            mx = mix.to(dt)
            inter = torch.empty(B * nq, mi.weight.shape[0], dtype=dt, device=h.device)
            engine.gemm(code, EPI_BIAS_GELU, mx, engine.CACHE.get(mi.weight, code), engine._f32c(mi.bias), inter)
            if rec:
                z = linear_f32(code, mx, mi.weight, mi.bias)             # the pre-GELU rows, for the backward only
            dense = linear_f32(code, inter, mo.weight, mo.bias)
            if rec:
                record.update({f"{l}.h": h, f"{l}.a": a, f"{l}.c": c, f"{l}.mix": mix, f"{l}.z": z,
                               f"{l}.inter": inter.float(), f"{l}.dense": dense})
            h = engine.residual_layernorm(dense, mix, layer.output_query.LayerNorm, self.eps)
        if rec:
            record["last"] = h
        return IQMOutput(h.view(B, nq, D))


def sinusoidal_positions(max_len: int, d_model: int) -> torch.Tensor:
    """reference model/adapter.py:98-105 -> [1, max_len, d_model]."""
    position = torch.arange(max_len, dtype=torch.float32).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d_model, 2, dtype=torch.float32) * (-math.log(10000.0) / d_model))
    pe = torch.zeros(max_len, d_model)
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe.unsqueeze(0)
