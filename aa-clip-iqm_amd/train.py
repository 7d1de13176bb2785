"""Stage 1 of training: fit the text adapters against frozen V-V ("surgery") patch features of CLIP, on the HIP path end
to end -- encode_text forward and backward (aaclip_hip.autograd.TextTower), the train-mode similarity map and the
segmentation loss with their backward kernels.  Behaviour follows reference train.py:57-113.

Of stage 2 (the image adapters) the loss is here: `stage2_text_loss`, the forward with a graph
(aaclip_hip.autograd.visual_heads) and the part of the loss that does not involve the IQM branch, and `stage2_loss`,
which adds the IQM map terms (aaclip_hip.autograd.iqm_map_train) for given final queries, with their gradient to the seg
tokens and to those queries.

Not here: the training-time datasets, main(), the backward of the IQM branch's 2-row query
side (the key / value side is built: aaclip_hip.autograd.cross_rows and iqm_visual_rows) and train_image_adapter.  `train_text_adapter` is fed by any
iterable of {"image", "mask", "class_name"} batches.
"""
from __future__ import annotations

import logging
import os

import torch
from torch import nn

import forward_utils as FU
from aaclip_hip import autograd

CHECKPOINT_NAME = "text_adapter.pth"
# reference train.py:131-132,156,163: the weight of the text-anchor maps against the IQM maps, and the two halvings
TEXT_WEIGHT = 0.6
IQM_WEIGHT = 0.4
CLS_LOSS_SCALE = 0.5
SEG_LOSS_SCALE = 0.5


def _unit(t: torch.Tensor) -> torch.Tensor:
    return t / t.norm(dim=-1, keepdim=True)


@torch.no_grad()
def stage1_patch_features(adapted_model, clip_surgery, image, levels=(6, 12, 18, 24)):
    """The frozen image side, one [B, P, E] tensor per tap level: the surgery model's tapped patch rows through ln_post
    and visual.proj as unit vectors, each shifted by the unit CLS embedding of the unmodified CLIP (not renormalised)."""
    visual = clip_surgery.visual
    taps = clip_surgery.encode_image(image, list(levels))[1]
    cls = _unit(adapted_model.clipmodel.encode_image(image, [])[0]).unsqueeze(1)
    return [_unit(visual.ln_post(tap[:, 1:, :]) @ visual.proj) + cls for tap in taps]


def batch_anchors(adapted_model, dataset_name, class_names, device):
    """[B, E, 2] anchor pairs of a batch; every distinct class is encoded once, with a graph down to the adapters."""
    per_class = {c: FU.get_adapted_single_class_text_embedding(adapted_model, dataset_name, c, device)
                 for c in set(class_names)}
    return torch.stack([per_class[c] for c in class_names])


def level_loss(features, anchors, mask, img_size, text_norm_weight):
    """Seg loss of one tap level plus text_norm_weight x (mean over the batch of <normal, abnormal>) squared."""
    seg = FU.calculate_seg_loss(FU.calculate_similarity_map(features, anchors, img_size), mask)
    overlap = (anchors[..., 0] * anchors[..., 1]).sum(dim=1).mean()
    return seg + text_norm_weight * overlap ** 2


def train_text_adapter(adapted_model: nn.Module, clip_surgery: nn.Module, text_norm_weight: float, train_loader,
                       optimizer: torch.optim.Optimizer, device: str, start_epoch: int, save_path: str, text_epoch: int,
                       dataset_name: str, img_size: int, logger: logging.Logger, levels=(6, 12, 18, 24)):
    """Same arguments as the reference's function (plus `levels`, which it hard-codes) and the same checkpoint after
    every epoch: {"epoch", "text_adapter", "text_optimizer"} in <save_path>/text_adapter.pth."""
    for epoch in range(start_epoch, text_epoch):
        logger.info(f"training text epoch {epoch}:")
        step_losses = []
        for batch in train_loader:
            mask = batch["mask"].to(device)
            anchors = batch_anchors(adapted_model, dataset_name, batch["class_name"], device)
            features = stage1_patch_features(adapted_model, clip_surgery, batch["image"].to(device), levels)
            # The reference overwrites its loss variable at every tap level, so what it back-propagates is the LAST
            # level's loss alone; the earlier levels are evaluated and discarded.  Kept as executed, quirk included.
            for level_features in features:
                loss = level_loss(level_features, anchors, mask, img_size, text_norm_weight)
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            step_losses.append(loss.item())
        logger.info(f"loss: {sum(step_losses) / len(step_losses)}")
        os.makedirs(save_path, exist_ok=True)
        torch.save({"epoch": epoch + 1, "text_adapter": adapted_model.text_adapter.state_dict(),
                    "text_optimizer": optimizer.state_dict()}, os.path.join(save_path, CHECKPOINT_NAME))
    return adapted_model


def stage2_text_loss(adapted_model, image, mask, label, anchors, img_size):
    """The stage-2 loss without its IQM terms (reference train.py:152-163), with a graph to the image adapters:
        CLS_LOSS_SCALE * cross_entropy((det.unsqueeze(1) @ anchors)[:, 0], label)
        + sum over the tap levels of TEXT_WEIGHT * SEG_LOSS_SCALE * seg_loss(similarity_map(seg, anchors), mask)
    image [B, 3, S, S], mask [B, 1, S, S] of 0 / 1, label [B] int64, anchors [B, E, 2] (the batch's text embeddings).
    The forward (autograd.visual_heads), the maps and the segmentation loss run on the HIP kernels, forward and backward;
    the [B, 2] matmul and cross-entropy of the classification term are host-side torch ops, like
    forward_utils.image_score.
    The IQM terms of the loss (train.py:165-212) are added by stage2_loss.  Not built: train_image_adapter (the epoch
    loop, clipping, scheduler and checkpoint around this loss)."""
    return _stage2_text_terms(adapted_model, image, mask, label, anchors, img_size)[0]


def _stage2_text_terms(adapted_model, image, mask, label, anchors, img_size):
    """-> (the loss of stage2_text_loss, the seg tokens it was computed from)"""
    seg_tokens, det = autograd.visual_heads(adapted_model, image)
    cls_preds = torch.matmul(det.unsqueeze(1), anchors)[:, 0]
    loss = CLS_LOSS_SCALE * nn.functional.cross_entropy(cls_preds, label)
    for seg in seg_tokens:
        preds = FU.calculate_similarity_map(seg, anchors, img_size)
        loss = loss + TEXT_WEIGHT * SEG_LOSS_SCALE * FU.calculate_seg_loss(preds, mask)
    return loss, seg_tokens


def iqm_map_loss(seg, iqm_queries, mask, img_size):
    """One tap level's IQM term (reference train.py:185-212): IQM_WEIGHT * SEG_LOSS_SCALE * seg_loss of the two-channel
    half-pixel upsample of (1 - p, p), p = sigmoid(cos(seg, q_abnormal) - cos(seg, q_normal))."""
    preds = autograd.iqm_map_train(seg, iqm_queries, img_size)
    return IQM_WEIGHT * SEG_LOSS_SCALE * FU.calculate_seg_loss(preds, mask)


def stage2_loss(adapted_model, image, mask, label, anchors, img_size, iqm_queries):
    """The stage-2 loss (reference train.py:152-212): stage2_text_loss plus, per tap level,
        IQM_WEIGHT * SEG_LOSS_SCALE * seg_loss(iqm_map_train(seg, iqm_queries, img_size), mask)
    iqm_queries [B, 2, E]: the IQM branch's final queries, row 0 normal and row 1 abnormal.  Any tensor of that shape
    serves; if it requires grad it receives its gradient (the input of the branch's backward), and the seg tokens pass
    theirs on to seg_proj and the layer adapters.  Until the branch has a backward the queries of a training step are
    model(image, text_embeddings=anchors)[2].last_hidden_state, which carries no graph: the branch's parameters do not
    train yet.
    A query width other than the seg tokens' raises ValueError: the reference draws a fresh random nn.Linear at every
    step there (train.py:175-179), which cannot be reproduced.
    Not built: the backward of the IQM branch's 2-row query side (from these queries' gradient to the effective queries
    of autograd.cross_rows; the key / value side behind them is autograd.iqm_visual_rows) and train_image_adapter."""
    E = adapted_model.image_adapter["seg_proj"][0].weight.shape[0]
    if iqm_queries.dim() != 3 or iqm_queries.shape[1] != 2 or iqm_queries.shape[-1] != E:
        raise ValueError(f"stage2_loss: iqm_queries must be [B, 2, {E}] (the seg tokens' width), got "
                         f"{tuple(iqm_queries.shape)}")
    loss, seg_tokens = _stage2_text_terms(adapted_model, image, mask, label, anchors, img_size)
    for seg in seg_tokens:
        loss = loss + iqm_map_loss(seg, iqm_queries, mask, img_size)
    return loss
