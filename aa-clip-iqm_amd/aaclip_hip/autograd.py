"""torch.autograd.Functions over the training entry points of libaaclip_hip.so (include/aaclip.h, "Training"): the
train-mode similarity map (reference forward_utils.py:196-216, test=False) and the segmentation loss (:21-108,223-227).
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


def similarity_map_train(seg, text_feature, img_size):
    return SimilarityMapTrain.apply(seg, text_feature, img_size)


def seg_loss(preds, mask, terms: int = _lib.SEG_LOSS_ALL):
    return SegLoss.apply(preds, mask, terms)
