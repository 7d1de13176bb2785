"""torch.autograd.Functions over the training entry points of libaaclip_hip.so (include/aaclip.h, "Training"): the
train-mode similarity map (reference forward_utils.py:196-216, test=False), the segmentation loss (:21-108,223-227) and
the adapted text tower (reference model/adapter.py:273-304), whose backward fills the text_adapter gradients, the
visual tower up to its tap streams (model/adapter.py:137-170), whose backward fills the layer-adapter gradients, and
the tap and det heads behind them (:171-184), whose backward fills the seg_proj / det_proj gradients, and the IQM map term of
the stage-2 loss (reference train.py:173-209: the two-channel half-pixel upsample of sigmoid(cos - cos)), whose backward
reaches the seg tokens and the two final queries.
Forward and backward are HIP kernels; these classes only carry tensors between them.  The saved tensors live in
ctx.save_for_backward, so they are freed with the graph (after backward(), or when the output is dropped)."""
from __future__ import annotations

import torch

from . import _lib, engine


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
    first trainable adapter's block on, and nothing else.  The backward runs in fp32 whatever precision the forward
    ran in: from the last tapped level down it adds d_tap into the running stream gradient at every tapped level and
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
                                            in_place=True)
            if aw is not None and ctx.needs_input_grad[2 + i]:
                grads[i] = d_aw.to(aw.dtype)
        return (None, None, *grads)


class TapHead(torch.autograd.Function):
    """One tap head of AdaptedCLIP.forward (reference model/adapter.py:171-184) with a backward for its projections and
    for the tap stream: ln_post and CLIP's other parameters are frozen, they are not inputs and receive no gradient.

    forward(model, tap [B, L, D], seg_proj weight, det_proj weight or None) -> seg [B, L-1, E], or (seg, det [B, E])
    with a det weight: exactly engine.tap_head at the model's precision, so the outputs do not depend on whether
    gradients are on.  Saved: the tap (the VisualTaps output itself, no copy) and the weights.  The backward is
    engine.tap_head_backward, fp32 whatever precision the forward ran in, recomputing the head from the tap; an output
    the loss does not read contributes nothing (its part is skipped), and a tap without a graph skips the
    input-gradient products."""

    @staticmethod
    def forward(ctx, model, tap, proj_weight, det_weight):
        B, L, D = tap.shape
        seg, det = engine.tap_head(tap.reshape(B * L, D), model.image_encoder.ln_post, proj_weight, model.relu, B, L,
                                   model._code(), det_weight=det_weight)
        ctx.model = model
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(tap, proj_weight, det_weight)
        return seg if det is None else (seg, det)

    @staticmethod
    def backward(ctx, d_seg, d_det=None):
        tap, pw, dw = ctx.saved_tensors
        _, need_x, need_p, need_d = ctx.needs_input_grad
        if (d_seg is None and d_det is None) or not (need_x or need_p or need_d):
            return None, None, None, None
        model = ctx.model
        d_x, d_pw, d_dw = engine.tap_head_backward(
            tap, model.image_encoder.ln_post, pw, _lib.ACT_LEAKY if model.relu else _lib.ACT_NONE, d_seg,
            det_weight=dw if d_det is not None else None, d_det=d_det, need_input_grad=need_x)
        return (None, d_x.view_as(tap).to(tap.dtype) if need_x else None,
                d_pw.to(pw.dtype) if need_p and d_pw is not None else None,
                d_dw.to(dw.dtype) if need_d and d_dw is not None else None)


def visual_taps(model, image):
    """The tap streams of AdaptedCLIP's visual tower, [B, L, D] each (CLS row included), one per entry of model.levels
    in ascending order, carrying a graph to model.image_adapter["layer_adapters"][i].weight: see VisualTaps.
    AdaptedCLIP.forward itself is unchanged and carries no graph; visual_heads puts the tap and det heads behind these
    streams with their HIP backward (TapHead), so a training step needs no torch-op composition of the heads."""
    return list(VisualTaps.apply(model, image, *[m.weight for m in model.image_adapter["layer_adapters"]]))


def visual_heads(model, image):
    """AdaptedCLIP.forward(image)[:2] with a graph -> (seg_tokens: one [B, L-1, E] tensor of unit rows per tap level,
    det_token [B, E]): visual_taps, then one TapHead per level with the det head on the last one, paired as the forward
    pairs them and bit-identical to it.  The graph reaches image_adapter["layer_adapters"][i].weight, ["seg_proj"][k]
    and ["det_proj"], whichever of them require grad.  Not built: the IQM branch's backward (the forward's third
    output); iqm_map_train hands it d_queries."""
    seg_proj = model.image_adapter["seg_proj"]
    det_weight = model.image_adapter["det_proj"].weight
    seg_tokens, det_token = [], None
    for k, tap in enumerate(visual_taps(model, image)):
        if k == len(model.levels) - 1:
            seg, det_token = TapHead.apply(model, tap, seg_proj[k].weight, det_weight)
        else:
            seg = TapHead.apply(model, tap, seg_proj[k].weight, None)
        seg_tokens.append(seg)
    return seg_tokens, det_token


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
