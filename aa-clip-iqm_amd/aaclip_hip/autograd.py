"""torch.autograd.Functions over the training entry points of libaaclip_hip.so (include/aaclip.h, "Training"): the
train-mode similarity map (reference forward_utils.py:196-216, test=False), the segmentation loss (:21-108,223-227) and
the adapted text tower (reference model/adapter.py:273-304), whose backward fills the text_adapter gradients, and the
visual tower up to its tap streams (model/adapter.py:137-170), whose backward fills the layer-adapter gradients.
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


def visual_taps(model, image):
    """The tap streams of AdaptedCLIP's visual tower, [B, L, D] each (CLS row included), one per entry of model.levels
    in ascending order, carrying a graph to model.image_adapter["layer_adapters"][i].weight: see VisualTaps.
    AdaptedCLIP.forward itself is unchanged and carries no graph; until the tap and det heads have backward kernels,
    a training step composes them from torch ops on the streams returned here (drop the CLS row, ln_post, seg_proj,
    normalise), as the tests do."""
    return list(VisualTaps.apply(model, image, *[m.weight for m in model.image_adapter["layer_adapters"]]))


def encode_text(model, tokens):
    """model.encode_text(tokens) with a graph: see TextTower."""
    return TextTower.apply(model, tokens, *[m.weight for m in model.text_adapter])


def similarity_map_train(seg, text_feature, img_size):
    return SimilarityMapTrain.apply(seg, text_feature, img_size)


def seg_loss(preds, mask, terms: int = _lib.SEG_LOSS_ALL):
    return SegLoss.apply(preds, mask, terms)
