"""torch.autograd.Functions over the training entry points of libaaclip_hip.so (include/aaclip.h, "Training"): the
train-mode similarity map (reference forward_utils.py:196-216, test=False), the segmentation loss (:21-108,223-227) and
the adapted text tower (reference model/adapter.py:273-304), whose backward fills the text_adapter gradients, the
visual tower up to its tap streams (model/adapter.py:137-170), whose backward fills the layer-adapter gradients, and
the tap and det heads behind them (:171-184), whose backward fills the seg_proj / det_proj gradients, and the IQM map term of
the stage-2 loss (reference train.py:173-209: the two-channel half-pixel upsample of sigmoid(cos - cos)), whose backward
reaches the seg tokens and the two final queries, and the key / value side of the IQM branch (model/adapter.py:205-211
and the visual cross-attention of model/iqm.py:108-139 over those rows): cross_rows and iqm_visual_rows, and the branch's
2-row query side (model/adapter.py:186-269, model/iqm.py:572-673) from the final queries back to every parameter it
reads, to those rows and to the CLS row of the last tap: IqmQueries / iqm_queries, visual_outputs.  That side has no
forward of its own here: IqmQueries runs the model's (AdaptedCLIP._iqm_branch) with a record of the intermediates.
iqm_train_form() "folded" selects IqmQueriesFolded instead: the same branch in the folded 16-bit form of inference
(aaclip_cross_rows_levels on the LayerNorm'ed tap rows), with aaclip_cross_rows_levels_backward behind it.
Forward and backward are HIP kernels; these classes only carry tensors between them.  The saved tensors live in
ctx.save_for_backward, so they are freed with the graph (after backward(), or when the output is dropped)."""
from __future__ import annotations

import torch

import contextlib
import os

from . import _lib, engine

# Arithmetic of the visual blocks' backward (VisualTaps): "fp32" (default, the exact-fp32 MFMA) or "bf16x3" (the
# three-term bf16 entries, include/aaclip.h "bf16x3").  The environment variable AACLIP_BACKWARD sets the initial value,
# in the manner of AACLIP_COMPUTE.  Forward outputs and losses do not depend on it; the text tower, the heads, the IQM
# branch and every row of at most 128 tokens keep their fp32 kernels whatever it says.
def backward_precision_from_env(environ=os.environ) -> str:
    """AACLIP_BACKWARD: unset or empty = fp32; an unknown value raises ValueError"""
    return engine.backward_precision_name(environ.get("AACLIP_BACKWARD") or "fp32")


_backward_precision = backward_precision_from_env()


def backward_precision() -> str:
    return _backward_precision


def set_backward_precision(mode) -> None:
    global _backward_precision
    _backward_precision = engine.backward_precision_name(mode)


@contextlib.contextmanager
def use_backward_precision(mode):
    """with use_backward_precision("bf16x3"): the graphs BUILT inside (VisualTaps.forward records the mode) run their
    visual-block backward in that arithmetic; the previous mode is restored on exit."""
    before = backward_precision()
    set_backward_precision(mode)
    try:
        yield
    finally:
        set_backward_precision(before)


# The form the IQM branch TRAINS in (iqm_queries, visual_outputs): "projected" (default: the projected key / value rows
# of IqmVisualRows + IqmQueries, whatever form inference takes) or "folded" (IqmQueriesFolded: the folded 16-bit form
# AdaptedCLIP.forward runs at the project's defaults, so that what is trained is what is served).  The environment
# variable AACLIP_IQM_TRAIN_FORM sets the initial value.
IQM_TRAIN_FORMS = ("projected", "folded")


def iqm_train_form_name(form) -> str:
    name = str(form).strip().lower()
    if name not in IQM_TRAIN_FORMS:
        raise ValueError(f"unknown IQM train form {form!r}: one of {IQM_TRAIN_FORMS}")
    return name


def iqm_train_form_from_env(environ=os.environ) -> str:
    """AACLIP_IQM_TRAIN_FORM: unset or empty = projected; an unknown value raises ValueError"""
    return iqm_train_form_name(environ.get("AACLIP_IQM_TRAIN_FORM") or "projected")


_iqm_train_form = iqm_train_form_from_env()


def iqm_train_form() -> str:
    return _iqm_train_form


def set_iqm_train_form(form) -> None:
    global _iqm_train_form
    _iqm_train_form = iqm_train_form_name(form)


@contextlib.contextmanager
def use_iqm_train_form(form):
    """with use_iqm_train_form("folded"): the graphs BUILT inside train the IQM branch in that form; the previous form
    is restored on exit."""
    before = iqm_train_form()
    set_iqm_train_form(form)
    try:
        yield
    finally:
        set_iqm_train_form(before)


class SimilarityMapTrain(torch.autograd.Function):
    """patch features [B,P,E] x anchors [E,2] or [B,E,2] -> softmax-over-anchors map [B,2,S,S]; the forward is the
    same kernel pair as engine.similarity_map_train, so the output does not depend on whether gradients are on."""

    @staticmethod
    def forward(ctx, seg, text_feature, img_size):
        out = engine.similarity_map_train(seg, text_feature, int(img_size))
        ctx.save_for_backward(seg, text_feature, out)
        return out

    @staticmethod
    def backward(ctx, d_out):
        seg, tf, out = ctx.saved_tensors
        need_seg, need_tf = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_seg or need_tf):
            return None, None, None
        d_seg, d_tf = engine.similarity_map_train_backward(seg, tf, out, d_out, need_seg=need_seg, need_anchors=need_tf)
        if d_tf is not None:
            d_tf = d_tf.to(tf.dtype)
        if d_seg is not None:
            d_seg = d_seg.to(seg.dtype)
        return d_seg, d_tf, None


class SegLoss(torch.autograd.Function):
    """preds + mask -> loss vector [4] = {focal + dice0 + dice1, focal, dice0, dice1} (terms not selected read 0).
    The mask takes no gradient (the reference's targets are data)."""

    @staticmethod
    def forward(ctx, preds, mask, terms):
        loss, coef = engine.seg_loss(preds, mask, terms)
        ctx.terms = terms
        ctx.save_for_backward(preds, mask, coef)
        return loss

    @staticmethod
    def backward(ctx, d_loss):
        preds, mask, coef = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        d = engine.seg_loss_backward(preds, mask, coef, d_loss, ctx.terms)
        return d.to(preds.dtype), None, None


class IqmMapTrain(torch.autograd.Function):
    """seg tokens [B,P,E] x final queries [B,2,E] (row 0 normal, row 1 abnormal) -> [B,2,S,S]: channel 1 the half-pixel
    bilinear upsample of p = sigmoid(cos(f, q_abnormal) - cos(f, q_normal)), channel 0 that of 1 - p.  The forward is
    engine.iqm_map_train, so the output does not depend on whether gradients are on; seg, the queries and the patch
    grid p are saved.  The backward computes only the gradients needs_input_grad asks for."""

    @staticmethod
    def forward(ctx, seg, queries, img_size):
        out, grid = engine.iqm_map_train(seg, queries, int(img_size))
        ctx.save_for_backward(seg, queries, grid)
        return out

    @staticmethod
    def backward(ctx, d_out):
        seg, q, grid = ctx.saved_tensors
        need_seg, need_q = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_seg or need_q):
            return None, None, None
        d_seg, d_q = engine.iqm_map_train_backward(seg, q, grid, d_out, need_seg=need_seg, need_queries=need_q)
        if d_seg is not None:
            d_seg = d_seg.to(seg.dtype)
        if d_q is not None:
            d_q = d_q.to(q.dtype)
        return d_seg, d_q, None


class TextTower(torch.autograd.Function):
    """AdaptedCLIP.encode_text with a backward for the text_adapter weights (CLIP's own parameters are frozen: they are
    not inputs of this Function and receive no gradient).

    forward(model, tokens, *text_adapter weights): the same kernels as the no-grad path, bit-identical embeddings; the
    tower runs as ONE aaclip_blocks_taps call that leaves the stream after every block in its own buffer.  Those
    layers x n*T x D fp32 values are all that is saved (ctx.save_for_backward: freed with the graph); the backward
    recomputes a block's internals from its input in fp32, whatever precision the forward ran in.  When only the last
    adapter (the EOT projection) requires grad, no block is revisited and only the n EOT rows are kept.
    The backward stops at the first block whose adapter requires grad (the token embedding is frozen)."""

    @staticmethod
    def forward(ctx, model, tokens, *weights):
        code = model._code()
        c = model.clipmodel
        until = model.text_adapt_until
        x0, tk = engine.text_embed(tokens, c.token_embedding.weight, c.positional_embedding)
        n, T = tk.shape
        blocks = list(c.transformer.resblocks)
        aws = [weights[i] if i < until else None for i in range(len(blocks))]
        need = [i for i in range(min(until, len(blocks))) if ctx.needs_input_grad[2 + i]]
        ctx.first = need[0] if need else None
        ctx.model, ctx.n, ctx.T = model, n, T
        if ctx.first is None:
            engine.run_blocks(x0, blocks, n, T, c.transformer.heads, code, causal=True, adapter_weights=aws, mix=model.t_w)
            out = engine.row_head(x0, tk, c.ln_final, weights[until], "plain", True, n, T, 0, code)
            eot = tk.argmax(dim=-1)
            ctx.save_for_backward(x0.view(n, T, -1)[torch.arange(n, device=x0.device), eot].contiguous(), tk, *weights)
            return out
        streams = torch.empty(len(blocks), n * T, x0.shape[1], dtype=torch.float32, device=x0.device)
        engine.run_blocks(x0, blocks, n, T, c.transformer.heads, code, causal=True, adapter_weights=aws, mix=model.t_w,
                          x_outs=[streams[i] for i in range(len(blocks))])
        out = engine.row_head(streams[-1], tk, c.ln_final, weights[until], "plain", True, n, T, 0, code)
        ctx.save_for_backward(streams, tk, *weights)
        return out

    @staticmethod
    def backward(ctx, d_out):
        saved, tk, *weights = ctx.saved_tensors
        model, n, T = ctx.model, ctx.n, ctx.T
        c = model.clipmodel
        until = model.text_adapt_until
        heads = c.transformer.heads
        grads = [None] * len(weights)
        d_out = d_out.contiguous().float()
        if ctx.first is None:
            # the n EOT rows as n one-row sequences: LayerNorm and the projection see rows, not sequences
            _, d_w = engine.row_head_backward(saved, None, c.ln_final, weights[until], _lib.ACT_LEAKY, d_out, n, 1, 1,
                                              need_input_grad=False)
            grads[until] = d_w.to(weights[until].dtype)
            return (None, None, *grads)
        blocks = list(c.transformer.resblocks)
        d_x, d_w = engine.row_head_backward(saved[-1], tk, c.ln_final, weights[until], _lib.ACT_LEAKY, d_out, n, T, 0)
        if ctx.needs_input_grad[2 + until]:
            grads[until] = d_w.to(weights[until].dtype)
        for i in range(len(blocks) - 1, ctx.first - 1, -1):
            if i > 0:
                x_in = saved[i - 1]
            else:   # the tower's input is not kept: token + positional embedding again
                x_in, _ = engine.text_embed(tk, c.token_embedding.weight, c.positional_embedding)
            aw = weights[i] if i < until else None
            _, d_aw = engine.block_backward(x_in, blocks[i], n, T, heads, d_x, causal=True, adapter_weight=aw,
                                            mix=model.t_w, need_input_grad=i > ctx.first, in_place=True)
            if aw is not None and ctx.needs_input_grad[2 + i]:
                grads[i] = d_aw.to(aw.dtype)
        return (None, None, *grads)


class VisualTaps(torch.autograd.Function):
    """The adapted visual tower up to its tap streams, with a backward for image_adapter["layer_adapters"] (CLIP's own
    parameters are frozen: they are not inputs of this Function and receive no gradient).

    forward(model, image, *layer-adapter weights) -> one stream [B, L, D] (CLS row included) per tapped level, in
    ascending order: engine.patch_embed, then the blocks up to the last tapped level as ONE aaclip_blocks_taps call
    that leaves the stream after every block in its own buffer -- the kernels of the no-grad path, so the taps are
    bit-identical to what AdaptedCLIP.forward feeds its heads.  Saved (ctx.save_for_backward: freed with the graph):
    the inputs of the blocks the backward revisits, i.e. the patch-embed output and the per-block streams from the
    first trainable adapter's block on, and nothing else.  The backward runs in fp32 (or, when
    backward_precision() said so at forward time, in bf16x3) whatever precision the forward ran in: from the last tapped level down it adds d_tap into the running stream gradient at every tapped level and
    calls engine.block_backward(in_place=True), which recomputes the block from its input; it stops at the first block
    whose adapter requires grad (the patch embedding is frozen).  Blocks above the last tapped level are never run.
    When no layer adapter requires grad nothing is saved."""

    @staticmethod
    def forward(ctx, model, image, *weights):
        code = model._code()
        v = model.image_encoder
        until = model.image_adapt_until
        all_blocks = list(v.transformer.resblocks)
        levels = [lv for lv in range(1, len(all_blocks) + 1) if lv in model.levels]
        if not levels:
            raise ValueError("visual_taps: model.levels names no block of the visual tower")
        blocks = all_blocks[:levels[-1]]
        if any(getattr(b, "surgery", False) for b in blocks):
            raise ValueError("visual_taps: the V-V attention blocks (DAPM_replace) have no backward")
        x0, B, L = engine.patch_embed(image, v, code)
        aws = [weights[i] if i < until else None for i in range(len(blocks))]
        outs = [torch.empty_like(x0) for _ in blocks]
        engine.run_blocks(x0, blocks, B, L, v.transformer.heads, code, causal=False, adapter_weights=aws, mix=model.i_w,
                          x_outs=outs)
        need = [i for i in range(min(until, len(blocks))) if ctx.needs_input_grad[2 + i]]
        ctx.first = need[0] if need else None
        ctx.model, ctx.B, ctx.L, ctx.levels = model, B, L, levels
        # rows of at most 128 tokens keep the stage-1 kernels whatever is selected
        ctx.precision = backward_precision() if L > engine.ATTN_BWD_SHORT_MAX_L else "fp32"
        if ctx.first is not None:
            ins = [x0] + outs[:-1]          # ins[i]: the input of block i
            ctx.save_for_backward(*ins[ctx.first:], *weights)
        return tuple(outs[lv - 1].view(B, L, -1) for lv in levels)

    @staticmethod
    def backward(ctx, *d_taps):
        model, B, L, levels = ctx.model, ctx.B, ctx.L, ctx.levels
        if ctx.first is None:
            return (None, None, *([None] * (len(ctx.needs_input_grad) - 2)))
        n_in = levels[-1] - ctx.first
        ins, weights = ctx.saved_tensors[:n_in], ctx.saved_tensors[n_in:]
        grads = [None] * len(weights)
        v = model.image_encoder
        blocks = list(v.transformer.resblocks)
        until = model.image_adapt_until
        d_x = None
        for i in range(levels[-1] - 1, ctx.first - 1, -1):
            if (i + 1) in levels:
                d_tap = d_taps[levels.index(i + 1)]
                if d_tap is not None:
                    d_tap = d_tap.reshape(B * L, -1).float()
                    d_x = d_tap.clone(memory_format=torch.contiguous_format) if d_x is None else d_x.add_(d_tap)
            if d_x is None:      # no gradient has entered the stream yet: this block's share is zero
                continue
            aw = weights[i] if i < until else None
            _, d_aw = engine.block_backward(ins[i - ctx.first], blocks[i], B, L, v.transformer.heads, d_x, causal=False,
                                            adapter_weight=aw, mix=model.i_w, need_input_grad=i > ctx.first,
                                            in_place=True, precision=ctx.precision)
            if aw is not None and ctx.needs_input_grad[2 + i]:
                grads[i] = d_aw.to(aw.dtype)
        return (None, None, *grads)


class TapHead(torch.autograd.Function):
    """One tap head of AdaptedCLIP.forward (reference model/adapter.py:171-184) with a backward for its projections and
    for the tap stream: ln_post and CLIP's other parameters are frozen, they are not inputs and receive no gradient.

    forward(model, tap [B, L, D], seg_proj weight, det_proj weight or None) -> seg [B, L-1, E], or (seg, det [B, E])
    with a det weight: exactly engine.tap_head at the model's precision, so the outputs do not depend on whether
    gradients are on.  A fifth argument keep_rows = True appends ln_post(tap) in the tower's 16-bit layout
    (engine.tap_head(keep_rows=True): what the folded IQM branch reads), marked non-differentiable.  Saved: the tap (the VisualTaps output itself, no copy) and the weights.  The backward is
    engine.tap_head_backward, fp32 whatever precision the forward ran in, recomputing the head from the tap; an output
    the loss does not read contributes nothing (its part is skipped), and a tap without a graph skips the
    input-gradient products."""

    @staticmethod
    def forward(ctx, model, tap, proj_weight, det_weight, keep_rows=False):
        B, L, D = tap.shape
        res = engine.tap_head(tap.reshape(B * L, D), model.image_encoder.ln_post, proj_weight, model.relu, B, L,
                              model._code(), det_weight=det_weight, keep_rows=bool(keep_rows))
        ctx.model, ctx.has_det = model, det_weight is not None
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(tap, proj_weight, det_weight)
        outs = (res[0],) + ((res[1],) if ctx.has_det else ())
        if keep_rows:                 # ln_post(tap) as the head wrote it: a constant for its readers, no gradient
            ctx.mark_non_differentiable(res[2])
            outs += (res[2],)
        return outs[0] if len(outs) == 1 else outs

    @staticmethod
    def backward(ctx, d_seg, *more):
        d_det = more[0] if ctx.has_det and more else None
        tap, pw, dw = ctx.saved_tensors
        _, need_x, need_p, need_d = ctx.needs_input_grad[:4]
        flag = (None,) * (len(ctx.needs_input_grad) - 4)          # keep_rows, when it was passed
        if (d_seg is None and d_det is None) or not (need_x or need_p or need_d):
            return (None, None, None, None) + flag
        model = ctx.model
        d_x, d_pw, d_dw = engine.tap_head_backward(
            tap, model.image_encoder.ln_post, pw, _lib.ACT_LEAKY if model.relu else _lib.ACT_NONE, d_seg,
            det_weight=dw if d_det is not None else None, d_det=d_det, need_input_grad=need_x)
        return (None, d_x.view_as(tap).to(tap.dtype) if need_x else None,
                d_pw.to(pw.dtype) if need_p and d_pw is not None else None,
                d_dw.to(dw.dtype) if need_d and d_dw is not None else None) + flag


class CrossRows(torch.autograd.Function):
    """engine.cross_rows with a backward: qt fp32 [B*R, Dk] x rows x [B*Lk, Dk] (fp32, fp16 or bf16) -> [B*R, Dk], the
    bits of the inference path.  Saved: qt and x themselves (nothing of size Lk x Dk is added; the backward recomputes
    the probabilities).  The backward is engine.cross_rows_backward, for the gradients needs_input_grad names only.
    act ACT_NONE: d x is the gradient with respect to the x given.  act ACT_LEAKY / ACT_RELU (x = that activation's
    output): the gradient handed back for x is already multiplied by the activation's slope, i.e. it is the gradient of
    the pre-activation rows -- what iqm_visual_rows(..., pre_activation_grad=True) expects to receive."""

    @staticmethod
    def forward(ctx, qt, x, B, R, Lk, act):
        code = {torch.float32: engine.F32, torch.float16: engine.F16, torch.bfloat16: engine.BF16}[x.dtype]
        qt32 = engine._f32c(qt)
        xr = x.detach().contiguous()
        out = engine.cross_rows(qt32, xr, int(B), int(R), int(Lk), code)
        ctx.dims = (int(B), int(R), int(Lk), code, int(act))
        ctx.save_for_backward(qt32, xr)
        return out.view(*qt.shape)

    @staticmethod
    def backward(ctx, d_out):
        qt, x = ctx.saved_tensors
        B, R, Lk, code, act = ctx.dims
        need_qt, need_x = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_qt or need_x):
            return None, None, None, None, None, None
        d_qt, d_x = engine.cross_rows_backward(qt, x.view(B * Lk, -1), d_out.reshape(B * R, -1), B, R, Lk, code, act=act,
                                               need_qt=need_qt, need_x=need_x)
        return (d_qt.view_as(d_out) if need_qt else None, d_x.view_as(x).to(x.dtype) if need_x else None,
                None, None, None, None)


class IqmVisualRows(torch.autograd.Function):
    """The key / value rows of the IQM branch in its projected form, [B, levels * (L - 1), h]: per tap level
    AdaptedCLIP._iqm_project_level (ln_post, query_adapters[k] with or without the LeakyReLU, CLS row dropped) -- the
    code and kernels AdaptedCLIP.forward runs, so the rows are its vis_cat bit for bit.

    forward(model, pre_activation_grad, n, *taps [B, L, D], *query_adapters weights).  Saved: the taps (the VisualTaps
    outputs themselves), the weights and, with the LeakyReLU, the output rows (their sign gives the slope).  The
    backward runs in fp32 whatever precision the forward ran in: ln_post(tap) again in fp32, the slope of the saved
    rows (skipped with pre_activation_grad: the incoming gradient is then that of the pre-activation product, as
    aaclip_cross_rows_backward with act set delivers it), aaclip_gemm_wgrad for d query_adapters[k].weight,
    aaclip_gemm on the transposed weight and aaclip_layernorm_backward for d tap (ln_post is frozen).  The CLS rows of
    d tap are exactly zero.  Level slices and the zero CLS row are torch copies."""

    @staticmethod
    def forward(ctx, model, pre_activation_grad, n, *tw):
        taps, weights = tw[:n], tw[n:]
        B, L, D = taps[0].shape
        icode = engine.plain_code(model._code())
        h = model.iqm_hidden_size
        vis_cat = torch.empty(B, n * (L - 1), h, dtype=engine.torch_dtype(icode), device=taps[0].device)
        for k, tap in enumerate(taps):
            model._iqm_project_level(tap.detach().reshape(B * L, D), k, vis_cat, B, L, icode)
        ctx.model, ctx.n, ctx.pre = model, n, bool(pre_activation_grad)
        ctx.save_for_backward(*taps, *weights, *([vis_cat] if model.relu and not ctx.pre else []))
        return vis_cat

    @staticmethod
    def backward(ctx, d_vis):
        model, n = ctx.model, ctx.n
        saved = ctx.saved_tensors
        taps, weights = saved[:n], saved[n:2 * n]
        B, L, D = taps[0].shape
        P = L - 1
        ln_post = model.image_encoder.ln_post
        grads_t, grads_w = [None] * n, [None] * n
        d_vis = d_vis.float()
        if model.relu and not ctx.pre:
            y = saved[2 * n]
            d_vis = d_vis * torch.where(y > 0, 1.0, 0.01).to(torch.float32)
        for k in range(n):
            need_t, need_w = ctx.needs_input_grad[3 + k], ctx.needs_input_grad[3 + n + k]
            if not (need_t or need_w):
                continue
            w = weights[k]
            dz = torch.zeros(B, L, w.shape[0], dtype=torch.float32, device=d_vis.device)   # CLS rows stay zero
            dz[:, 1:, :] = d_vis[:, k * P:(k + 1) * P, :]
            dz = dz.view(B * L, -1)
            tap32 = engine._f32c(taps[k]).reshape(B * L, D)
            if need_w:
                ln = engine.layernorm(tap32, ln_post.weight, ln_post.bias, out_code=engine.F32)
                grads_w[k] = engine.gemm_wgrad(dz, ln).to(w.dtype)
            if need_t:
                d_ln = torch.empty(B * L, D, dtype=torch.float32, device=d_vis.device)
                engine.gemm(engine.F32, _lib.EPI_ACT_F32, dz, engine.CACHE.get(w, engine.F32, "transpose"), None, d_ln)
                d_tap = engine.layernorm_backward(tap32, ln_post.weight, d_ln).view(B, L, D)
                d_tap[:, 0, :] = 0.0
                grads_t[k] = d_tap.to(taps[k].dtype)
        return (None, None, None, *grads_t, *grads_w)


_ATTENTIONS = ("attention", "crossattention", "text_crossattention")


def _iqm_param_names(model):
    """The parameters the query side of the IQM branch reads, by their state_dict names, in the order IqmQueries takes
    them (IQMLayer.intermediate / .output, visual_weight and text_weight are not read and are not here)."""
    names = [f"class_query_mlp.{i}.{p}" for i in (0, 2) for p in ("weight", "bias")] + ["pos_embedding"]
    names += ["iqm.layernorm.weight", "iqm.layernorm.bias"]
    for l in range(len(model.iqm.encoder.layer)):
        pre = f"iqm.encoder.layer.{l}."
        for att in _ATTENTIONS:
            for m in ("attention.query", "attention.key", "attention.value", "output.dense", "output.LayerNorm"):
                names += [f"{pre}{att}.{m}.weight", f"{pre}{att}.{m}.bias"]
        for m in ("intermediate_query.dense", "output_query.dense", "output_query.LayerNorm"):
            names += [f"{pre}{m}.weight", f"{pre}{m}.bias"]
    for m in ("visual_feature_proj", "text_feature_proj", "iqm_layer_norm"):
        names += [m + ".weight", m + ".bias"]
    return names


def _iqm_train_check(model):
    """The configurations IqmQueries covers: the last tap is the tower's final stream, and both cross-attentions take
    the aaclip_cross_rows form of IQM._attend.  With iqm_train_form() "folded" (IqmQueriesFolded) the model's forward
    must fold as well (AdaptedCLIP.iqm_folds_levels); the text cross-attention keeps its aaclip_cross_rows form."""
    if iqm_train_form() == "folded" and not model.iqm_folds_levels():
        raise NotImplementedError("iqm_queries: the IQM train form is \"folded\", but this model's forward does not fold "
                                  "(AdaptedCLIP.iqm_folds_levels: a 16-bit tower 768 or 1024 wide, no LeakyReLU in "
                                  "query_adapters, at most 4 tap levels, at most 8 heads)")
    n_blocks = len(model.image_encoder.transformer.resblocks)
    if not model.levels or max(model.levels) != n_blocks:
        raise NotImplementedError("iqm_queries: model.levels must end at the tower's last block (the CLS row of the final "
                                  "stream is read from the last tap)")
    widths = (model.iqm_hidden_size, model.text_feature_proj.weight.shape[0])
    if not all(model.iqm.cross_rows_form(2, w) for w in widths):
        raise NotImplementedError("iqm_queries: training covers queries x heads in {4, 8, 12, 16} and row widths "
                                  "256 / 512 / 768 / 1024 (the aaclip_cross_rows form of the cross-attentions)")


def _dx(d_y, weight):
    """d_y [M, out] . W [out, in] -> [M, in] fp32: the input gradient of x W^T"""
    out = torch.empty(d_y.shape[0], weight.shape[1], dtype=torch.float32, device=d_y.device)
    return engine.gemm(engine.F32, _lib.EPI_ACT_F32, d_y, engine.CACHE.get(weight, engine.F32, "transpose"), None, out)


def _dx_t(d_y, weight):
    """d_y [M, in] . W^T -> [M, out] fp32: the input gradient of x W (a product that ran on the transposed weight)"""
    out = torch.empty(d_y.shape[0], weight.shape[0], dtype=torch.float32, device=d_y.device)
    return engine.gemm(engine.F32, _lib.EPI_ACT_F32, d_y, engine.CACHE.get(weight, engine.F32), None, out)


def _wgrad(dz, u):
    """aaclip_gemm_wgrad over column blocks of at most 1024 output features of dz"""
    O = dz.shape[1]
    if O <= 1024:
        return engine.gemm_wgrad(dz, u)
    return torch.cat([engine.gemm_wgrad(dz[:, o:o + 1024], u) for o in range(0, O, 1024)], dim=0)


def _sum(a, b, c=None):
    return engine.combine3(a, b, c, 1.0, 1.0, 1.0)


def _iqm_query_walk(model, names, S, B, Lt, code, wanted, d_out, rows_step):
    """The backward walk of the IQM branch's 2-row query side, shared by the projected and the folded form: from d_out
    [B, 2, h] in reverse through AdaptedCLIP._iqm_branch / IQM.forward on the record S, for the parameters `wanted` (a
    set of the names in `names`).  rows_step(key, d_xbar) -> d_qx is the one step that differs: the visual
    cross-attention's weighted rows, from the gradient of xbar (the input of visual_feature_proj on the way out) to the
    gradient of qx (qt times visual_feature_proj's weight on the way in); it keeps the key / value side's gradients to
    itself.  -> (G: name -> fp32 gradient, d_cls [B, D]: the gradient of the CLS rows of the last tap)."""
    from ._lib import ACT_GELU, ACT_RELU
    iqm, h, H = model.iqm, model.iqm_hidden_size, model.iqm.num_attention_heads
    nq, R, eps = 2, 2 * H, iqm.eps
    scale = 1.0 / (h // H) ** 0.5
    need_txt = bool({"text_feature_proj.weight", "text_feature_proj.bias"} & wanted)
    G = {}
    buf = {"txt": None}

    def linear_params(name, dz, u):
        if name + ".weight" in wanted:
            G[name + ".weight"] = _wgrad(dz, u)
        if name + ".bias" in wanted:
            G[name + ".bias"] = engine.bias_grad(dz)

    def ln_bwd(name, ln, x, d_y, e):
        if name + ".weight" in wanted or name + ".bias" in wanted:
            G[name + ".weight"], G[name + ".bias"] = engine.layernorm_param_grad(x, d_y, e)
        return engine.layernorm_backward(x, ln.weight, d_y, eps=e)

    def tail_bwd(name, att, key, hin, d_y):
        """-> (d of the residual input, d ctx)"""
        s = engine.combine3(S[key + "dense"], hin, None, 1.0, 1.0, 0.0)
        d_s = ln_bwd(name + "output.LayerNorm", att.output.LayerNorm, s, d_y, eps)
        linear_params(name + "output.dense", d_s, S[key + "ctx"])
        return d_s, _dx(d_s, att.output.dense.weight)

    def self_bwd(name, att, key, hin, d_y):
        d_h, d_ctx = tail_bwd(name, att, key, hin, d_y)
        d_q, d_k, d_v = engine.small_attention_backward(S[key + "q"], S[key + "k"], S[key + "v"], d_ctx, B, nq, nq, H)
        for m, dz in (("query", d_q), ("key", d_k), ("value", d_v)):
            linear_params(f"{name}attention.{m}", dz, hin)
        d_h = _sum(d_h, _dx(d_q, att.attention.query.weight), _dx(d_k, att.attention.key.weight))
        return _sum(d_h, _dx(d_v, att.attention.value.weight))

    def cross_bwd(name, att, key, hin, proj, d_y):
        d_h, d_ctx = tail_bwd(name, att, key, hin, d_y)
        d_full = engine.head_expand(d_ctx, H, 1.0, engine.F32)             # the gradient of head_diag
        linear_params(name + "attention.value", d_full, S[key + "ebar"])
        d_ebar = _dx(d_full, att.attention.value.weight)
        qt = S[key + "qt"]
        if proj is not None:
            pname = "visual_feature_proj"
            if pname + ".weight" in wanted:                                # ebar = xbar P^T + b_p
                G.setdefault(pname + ".weight", []).append(_wgrad(d_ebar, S[key + "xbar"]))
            if pname + ".bias" in wanted:
                G.setdefault(pname + ".bias", []).append(engine.bias_grad(d_ebar))
            d_qx = rows_step(key, _dx(d_ebar, proj.weight))
            if pname + ".weight" in wanted:                                # qx = qt P
                G[pname + ".weight"].append(_wgrad(qt, d_qx))
            d_qt = _dx_t(d_qx, proj.weight)
        else:
            d_qt, buf["txt"] = engine.cross_rows_backward(qt, S["txt"], d_ebar, B, R, Lt, code, need_x=need_txt,
                                                          d_x=buf["txt"])
        kname = name + "attention.key"
        if kname + ".weight" in wanted:                                    # qt = qm W_k
            G[kname + ".weight"] = _wgrad(S[key + "qm"], d_qt)
        if kname + ".bias" in wanted:                                      # softmax-invariant
            G[kname + ".bias"] = torch.zeros_like(att.attention.key.bias, dtype=torch.float32)
        d_qm = _dx_t(d_qt, att.attention.key.weight)
        d_q = engine.combine3(engine.head_diag(d_qm, H), None, None, scale, 0.0, 0.0)   # the gradient of head_expand
        linear_params(name + "attention.query", d_q, hin)
        return _sum(d_h, _dx(d_q, att.attention.query.weight))

    d = engine._f32c(d_out).reshape(B * nq, h)
    d = ln_bwd("iqm_layer_norm", model.iqm_layer_norm, S["last"], d, model.iqm_layer_norm.eps)
    vp = model.visual_feature_proj
    for l in range(len(iqm.encoder.layer) - 1, -1, -1):
        layer, key, name = iqm.encoder.layer[l], f"{l}.", f"iqm.encoder.layer.{l}."
        mix, a, c, hin = S[key + "mix"], S[key + "a"], S[key + "c"], S[key + "h"]
        s = engine.combine3(S[key + "dense"], mix, None, 1.0, 1.0, 0.0)
        d_s = ln_bwd(name + "output_query.LayerNorm", layer.output_query.LayerNorm, s, d, eps)
        linear_params(name + "output_query.dense", d_s, S[key + "inter"])
        d_z = engine.act_backward(ACT_GELU, S[key + "z"], _dx(d_s, layer.output_query.dense.weight), in_place=True)
        linear_params(name + "intermediate_query.dense", d_z, mix)
        d_mix = _sum(d_s, _dx(d_z, layer.intermediate_query.dense.weight))
        d_c = cross_bwd(name + "text_crossattention.", layer.text_crossattention, key + "t.", c, None,
                        engine.combine3(d_mix, None, None, 0.3, 0.0, 0.0))
        d_a = cross_bwd(name + "crossattention.", layer.crossattention, key + "c.", a, vp,
                        engine.combine3(d_mix, d_c, None, 0.3, 1.0, 0.0))
        d = self_bwd(name + "attention.", layer.attention, key + "a.", hin,
                     engine.combine3(d_mix, d_a, None, 0.4, 1.0, 0.0))
    d_query = ln_bwd("iqm.layernorm", iqm.layernorm, S["query"].reshape(B * nq, h), d, eps)
    if "pos_embedding" in wanted:
        g = torch.zeros_like(model.pos_embedding, dtype=torch.float32)
        g[:, :2, :] = engine.bias_grad(d_query.view(B, 2 * h)).view(1, 2, h)
        G["pos_embedding"] = g
    dq3 = d_query.view(B, 2, h)
    d_cq = _sum(dq3[:, 0, :].contiguous(), dq3[:, 1, :].contiguous())
    m0, m2 = model.class_query_mlp[0], model.class_query_mlp[2]
    linear_params("class_query_mlp.2", d_cq, S["t1"])
    d_z1 = engine.act_backward(ACT_RELU, S["t1"], _dx(d_cq, m2.weight), in_place=True)
    linear_params("class_query_mlp.0", d_z1, S["cls"])
    if need_txt:
        d_w, d_b = engine.linear_smallk_backward(S["te"], buf["txt"])
        G["text_feature_proj.weight"], G["text_feature_proj.bias"] = d_w, d_b
    for n in ("visual_feature_proj.weight", "visual_feature_proj.bias"):   # fixed order: layer by layer, last first
        if G.get(n):
            G[n] = _sum_in_order(G[n])
    return G, (lambda: _dx(d_z1, m0.weight))


def _sum_in_order(parts):
    total = parts[0]
    for p in parts[1:]:
        total = _sum(total, p)
    return total


def _param_grads(model, names, wanted, G):
    params = dict(model.named_parameters())
    return [G[n].view_as(params[n]).to(params[n].dtype) if n in wanted else None for n in names]


class IqmQueries(torch.autograd.Function):
    """The query side of the IQM branch in its projected form with a backward:
    forward(model, rows, tap, anchors, *parameters named by _iqm_param_names) -> final queries [B, 2, h].
    rows [B, Lk, h] are autograd.iqm_visual_rows(model, taps, pre_activation_grad=model.relu), tap [B, L, D] the last tap
    stream (its CLS row feeds class_query_mlp), anchors [B, 768, 2] constants.  The forward IS the model's:
    AdaptedCLIP._iqm_branch(..., levels=None, record=S), the code AdaptedCLIP.forward runs, so wherever that takes the
    projected form the queries are its bits.  Saved: the record S and nothing else -- IQM.forward (model/iqm.py) lists
    its keys: the fp32 intermediates of every step ([2B, h], [2B H, .], the [2B, 2048] pre-GELU rows from one extra
    EPI_ACT_F32 product), the text rows and the rows tensor itself, nothing else of size Lk x h.
    The backward runs in fp32 whatever precision the forward ran in (16-bit casts count as the identity) and walks the
    forward in reverse on aaclip_gemm (transposed cached weights), aaclip_gemm_wgrad, aaclip_layernorm_backward,
    aaclip_cross_rows_backward (accumulating over roles and layers; its act applies the LeakyReLU slope of the rows) and
    the entries of csrc/iqm_query_backward.hip.  key.bias of both cross-attentions is softmax-invariant: exact zeros."""

    @staticmethod
    def forward(ctx, model, rows, tap, anchors, *params):
        code = engine.plain_code(model._code())
        B, L, _ = tap.shape
        if anchors.dim() != 3 or anchors.shape[0] != B or anchors.shape[-1] != 2:
            raise NotImplementedError("iqm_queries: text_embeddings must be [B, 768, 2]")
        S = {}
        out = model._iqm_branch(tap.detach(), rows.detach(), anchors.detach(), B, L, code, levels=None, record=S)
        ctx.model, ctx.keys, ctx.dims = model, list(S), (B, L, rows.shape[1], anchors.shape[1], code)
        ctx.names = _iqm_param_names(model)
        ctx.save_for_backward(*S.values())
        return out.last_hidden_state

    @staticmethod
    def backward(ctx, d_out):
        from ._lib import ACT_LEAKY, ACT_NONE
        model, names = ctx.model, ctx.names
        B, L, Lv, Lt, code = ctx.dims
        S = dict(zip(ctx.keys, ctx.saved_tensors))
        R = 2 * model.iqm.num_attention_heads
        wanted = {n for i, n in enumerate(names) if ctx.needs_input_grad[4 + i]}
        need_rows, need_tap = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        act = ACT_LEAKY if model.relu else ACT_NONE
        buf = {"rows": None}

        def rows_step(key, d_xbar):
            d_qx, buf["rows"] = engine.cross_rows_backward(S[key + "qx"], S["vis"], d_xbar, B, R, Lv, code, act=act,
                                                           need_x=need_rows, d_x=buf["rows"])
            return d_qx

        G, d_cls = _iqm_query_walk(model, names, S, B, Lt, code, wanted, d_out, rows_step)
        d_tap = None
        if need_tap:
            d_tap = torch.zeros(B, L, model.class_query_mlp[0].weight.shape[1], dtype=torch.float32, device=d_out.device)
            d_tap[:, 0, :] = d_cls()
        d_rows = buf["rows"].view(B, Lv, -1) if need_rows else None
        return (None, d_rows, d_tap, None, *_param_grads(model, names, wanted, G))


class IqmQueriesFolded(torch.autograd.Function):
    """The IQM branch in the folded 16-bit form AdaptedCLIP.forward runs at the project's defaults, with a backward:
    forward(model, n, anchors, *taps, *rows, *query_adapters weights, *parameters named by _iqm_param_names) -> final
    queries [B, 2, h].  taps: the n tap streams [B, L, D] (visual_taps); rows: ln_post of them in the tower's 16-bit
    layout, the very buffers engine.tap_head(keep_rows=True) wrote (constants here: their gradient is returned for the
    taps).  The forward IS the model's: AdaptedCLIP._iqm_levels and _iqm_branch(..., levels, record=S), so the queries
    are AdaptedCLIP.forward's bits.  Saved: the record (IQM.forward lists its keys: 2-row and [2 B H, .] intermediates),
    the taps, the rows and the weights -- nothing of size Lk x D is added to what the heads keep anyway.
    The backward runs in fp32 on the 16-bit row values as they are (other 16-bit casts count as the identity): the
    query-side walk of IqmQueries with the visual cross-attention's step replaced by
        d_xbar -> d tbar = d_xbar W_out,  d W_qa[s] += d_xbar^T tbar[., s]        (xbar = sum_s tbar[., s] W_qa[s]^T)
        aaclip_cross_rows_levels_backward -> d_u and, accumulated over the layers, d ln rows per level
        d W_qa[s] += qx^T d_u[., s],  d_qx = sum_s d_u[., s] W_qa[s]^T           (u[., s] = qx W_qa[s])
    and d tap[k] = aaclip_layernorm_backward of ln_post on the d ln rows (CLS rows exactly zero; the last tap's CLS rows
    then take class_query_mlp's share).  Sums over layers and roles run in a fixed order: last layer first, and within a
    layer the way out (xbar) before the way in (u)."""

    @staticmethod
    def forward(ctx, model, n, anchors, *tensors):
        taps, rows, qa = tensors[:n], tensors[n:2 * n], tensors[2 * n:3 * n]
        code = engine.plain_code(model._code())
        B, L, _ = taps[0].shape
        if anchors.dim() != 3 or anchors.shape[0] != B or anchors.shape[-1] != 2:
            raise NotImplementedError("iqm_queries: text_embeddings must be [B, 768, 2]")
        levels = model._iqm_levels([r.detach() for r in rows], L, code)
        S = {}
        out = model._iqm_branch(taps[-1].detach(), None, anchors.detach(), B, L, code, levels=levels, record=S)
        S.pop("vis")                                     # the levels dict: its row buffers are saved below
        ctx.model, ctx.n, ctx.keys, ctx.dims = model, n, list(S), (B, L, anchors.shape[1], code)
        ctx.names = _iqm_param_names(model)
        ctx.save_for_backward(*S.values(), *taps, *rows, *qa)
        return out.last_hidden_state

    @staticmethod
    def backward(ctx, d_out):
        model, names, n = ctx.model, ctx.names, ctx.n
        B, L, Lt, code = ctx.dims
        saved = ctx.saved_tensors
        nk = len(ctx.keys)
        S = dict(zip(ctx.keys, saved[:nk]))
        taps, rows, qa = saved[nk:nk + n], saved[nk + n:nk + 2 * n], saved[nk + 2 * n:nk + 3 * n]
        R = 2 * model.iqm.num_attention_heads
        D, h = qa[0].shape[1], qa[0].shape[0]
        need_taps = [ctx.needs_input_grad[3 + k] for k in range(n)]
        need_qa = [ctx.needs_input_grad[3 + 2 * n + k] for k in range(n)]
        wanted = {nm for i, nm in enumerate(names) if ctx.needs_input_grad[3 + 3 * n + i]}
        w_in = torch.cat([w.detach().float().t() for w in qa], 0).contiguous()           # [n*D, h]
        w_out = torch.cat([w.detach().float() for w in qa], 1).contiguous()              # [h, n*D]
        d_ln = None                                                                      # per level [B*L, D]
        parts = [[] for _ in range(n)]

        def rows_step(key, d_xbar):
            nonlocal d_ln
            M = d_xbar.shape[0]
            tbar, qx = S[key + "tbar"], S[key + "qx"]
            for k in range(n):
                if need_qa[k]:
                    parts[k].append(_wgrad(d_xbar, tbar[:, k * D:(k + 1) * D]))
            d_tbar = torch.empty(M, n * D, dtype=torch.float32, device=d_xbar.device)
            engine.gemm(engine.F32, _lib.EPI_ACT_F32, d_xbar, w_in, None, d_tbar)
            d_u, d_ln = engine.cross_rows_levels_backward(S[key + "u"], list(rows), d_tbar, B, R, L, 1, L - 1, D,
                                                          need_x=any(need_taps), d_x=d_ln)
            for k in range(n):
                if need_qa[k]:
                    parts[k].append(_wgrad(qx, d_u[:, k * D:(k + 1) * D]))
            d_qx = torch.empty(M, h, dtype=torch.float32, device=d_xbar.device)
            return engine.gemm(engine.F32, _lib.EPI_ACT_F32, d_u, w_out, None, d_qx)

        G, d_cls = _iqm_query_walk(model, names, S, B, Lt, code, wanted, d_out, rows_step)
        ln_post = model.image_encoder.ln_post
        d_taps = [None] * n
        for k in range(n):
            if need_taps[k]:
                tap32 = engine._f32c(taps[k]).reshape(B * L, D)
                d_tap = engine.layernorm_backward(tap32, ln_post.weight, d_ln[k]).view(B, L, D)
                d_tap[:, 0, :] = 0.0
                if k == n - 1:
                    d_tap[:, 0, :] = d_cls()
                d_taps[k] = d_tap.to(taps[k].dtype)
        d_qa = [_sum_in_order(parts[k]).to(qa[k].dtype) if need_qa[k] else None for k in range(n)]
        return (None, None, None, *d_taps, *([None] * n), *d_qa, *_param_grads(model, names, wanted, G))


def visual_taps(model, image):
    """The tap streams of AdaptedCLIP's visual tower, [B, L, D] each (CLS row included), one per entry of model.levels
    in ascending order, carrying a graph to model.image_adapter["layer_adapters"][i].weight: see VisualTaps.
    AdaptedCLIP.forward itself is unchanged and carries no graph; visual_heads puts the tap and det heads behind these
    streams with their HIP backward (TapHead), so a training step needs no torch-op composition of the heads."""
    return list(VisualTaps.apply(model, image, *[m.weight for m in model.image_adapter["layer_adapters"]]))


def visual_heads(model, image, taps=None, keep_rows=False):
    """AdaptedCLIP.forward(image)[:2] with a graph -> (seg_tokens: one [B, L-1, E] tensor of unit rows per tap level,
    det_token [B, E]): visual_taps, then one TapHead per level with the det head on the last one, paired as the forward
    pairs them and bit-identical to it.  The graph reaches image_adapter["layer_adapters"][i].weight, ["seg_proj"][k]
    and ["det_proj"], whichever of them require grad.  taps: the streams of a visual_taps(model, image) call the caller
    has already made (visual_outputs shares them with the IQM branch); None computes them here.
    keep_rows: -> (seg_tokens, det_token, rows) with rows[k] = ln_post(tap k) as the head wrote it in the tower's 16-bit
    layout (engine.tap_head(keep_rows=True)): what the folded IQM branch reads, without a second pass over the taps."""
    seg_proj = model.image_adapter["seg_proj"]
    det_weight = model.image_adapter["det_proj"].weight
    seg_tokens, det_token, rows = [], None, []
    for k, tap in enumerate(visual_taps(model, image) if taps is None else taps):
        last = k == len(model.levels) - 1
        res = TapHead.apply(model, tap, seg_proj[k].weight, det_weight if last else None, *([True] if keep_rows else []))
        res = res if isinstance(res, tuple) else (res,)
        seg_tokens.append(res[0])
        if last:
            det_token = res[1]
        if keep_rows:
            rows.append(res[-1])
    return (seg_tokens, det_token, rows) if keep_rows else (seg_tokens, det_token)


def iqm_queries(model, taps, anchors, rows=None):
    """The IQM branch's final queries [B, 2, h] = AdaptedCLIP.forward(image, anchors)[2].last_hidden_state, with a graph
    to every parameter the branch reads (model.iqm, class_query_mlp, visual_feature_proj, text_feature_proj,
    iqm_layer_norm, pos_embedding[:, :2]), to query_adapters and, through the taps [B, L, D] (from visual_taps), to
    layer_adapters: iqm_visual_rows for the key / value rows, IqmQueries for the 2-row query side.  The anchors
    [B, 768, 2] take no gradient.  NotImplementedError (before any launch): model.levels does not end at the tower's
    last block, or a configuration outside the aaclip_cross_rows form (see _iqm_train_check).
    With iqm_train_form() "folded" the branch runs and trains in the folded 16-bit form of AdaptedCLIP.forward
    (IqmQueriesFolded) -- same destinations, same bits as inference; NotImplementedError before any launch when the
    model's forward does not fold.  rows (folded form only): ln_post of the taps as visual_heads(keep_rows=True)
    returned them; None runs engine.tap_head(keep_rows=True) on the taps here."""
    _iqm_train_check(model)
    taps = list(taps)
    params = dict(model.named_parameters())
    if iqm_train_form() == "folded":
        if rows is None:
            B, L, D = taps[0].shape
            rows = [engine.tap_head(t.detach().reshape(B * L, D), model.image_encoder.ln_post, sp.weight, model.relu, B,
                                    L, model._code(), keep_rows=True)[2]
                    for t, sp in zip(taps, model.image_adapter["seg_proj"])]
        return IqmQueriesFolded.apply(model, len(taps), anchors, *taps, *rows, *[m.weight for m in model.query_adapters],
                                      *[params[n] for n in _iqm_param_names(model)])
    rows = iqm_visual_rows(model, taps, pre_activation_grad=model.relu)
    return IqmQueries.apply(model, rows, taps[-1], anchors, *[params[n] for n in _iqm_param_names(model)])


def visual_outputs(model, image, anchors):
    """AdaptedCLIP.forward(image, text_embeddings=anchors) with a graph -> (seg_tokens, det_token, queries [B, 2, h])
    from ONE visual_taps call: visual_heads and iqm_queries on the same tap streams.  In the folded train form the
    branch reads the LayerNorm'ed rows the heads wrote: neither the tower nor the heads run twice."""
    _iqm_train_check(model)
    taps = visual_taps(model, image)
    if iqm_train_form() == "folded":
        seg_tokens, det_token, rows = visual_heads(model, image, taps=taps, keep_rows=True)
        return seg_tokens, det_token, iqm_queries(model, taps, anchors, rows=rows)
    seg_tokens, det_token = visual_heads(model, image, taps=taps)
    return seg_tokens, det_token, iqm_queries(model, taps, anchors)


def encode_text(model, tokens):
    """model.encode_text(tokens) with a graph: see TextTower."""
    return TextTower.apply(model, tokens, *[m.weight for m in model.text_adapter])


def similarity_map_train(seg, text_feature, img_size):
    return SimilarityMapTrain.apply(seg, text_feature, img_size)


def iqm_map_train(seg, queries, img_size):
    """The IQM map of one tap level for the stage-2 loss, [B, 2, S, S], with a graph to seg and to the queries: see
    IqmMapTrain."""
    return IqmMapTrain.apply(seg, queries, img_size)


def seg_loss(preds, mask, terms: int = _lib.SEG_LOSS_ALL):
    return SegLoss.apply(preds, mask, terms)



def cross_rows(qt, x, B, R, Lk, act=None):
    """engine.cross_rows with a graph to qt and x: see CrossRows.  act None: the plain gradient."""
    return CrossRows.apply(qt, x, B, R, Lk, _lib.ACT_NONE if act is None else int(act))


def iqm_visual_rows(model, taps, pre_activation_grad=False):
    """The concatenated key / value rows [B, levels * (L - 1), h] of the IQM branch (the vis_cat of the projected form of
    AdaptedCLIP.forward, bit for bit) with a graph to every query_adapters[k].weight and to the tap streams
    taps[k] [B, L, D] (from visual_taps, so the graph reaches layer_adapters): see IqmVisualRows.
    pre_activation_grad: the gradient that arrives is already that of the pre-activation product (CrossRows with act
    set, or aaclip_cross_rows_backward with act), so the LeakyReLU slope is not applied again."""
    taps = list(taps)
    if len(taps) != len(model.query_adapters):
        raise ValueError("iqm_visual_rows: one tap stream per query adapter")
    return IqmVisualRows.apply(model, bool(pre_activation_grad), len(taps), *taps,
                               *[m.weight for m in model.query_adapters])
