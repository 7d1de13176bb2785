"""Training on the HIP path end to end.

Stage 1 (reference train.py:57-113) fits the text adapters against frozen V-V ("surgery") patch features of CLIP:
encode_text forward and backward (aaclip_hip.autograd.TextTower), the train-mode similarity map and the segmentation
loss with their backward kernels.  `train_text_adapter` is fed by any iterable of {"image", "mask", "class_name"}
batches.

Stage 2 (reference train.py:117-237) fits the image adapters and the IQM branch: `stage2_loss` is the reference's loss
-- the classification term, the text-anchor maps and the IQM maps -- on one forward with a graph
(aaclip_hip.autograd.visual_outputs: tap streams, tap / det heads and the IQM branch's final queries, each with its HIP
backward), and `train_image_adapter` is the reference's epoch loop around it.

Not here: the training-time datasets and main().
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
    The IQM terms of the loss (train.py:165-212) are added by stage2_loss."""
    return _stage2_text_terms(adapted_model, image, mask, label, anchors, img_size)[0]


def _stage2_text_terms(adapted_model, image, mask, label, anchors, img_size, heads=None):
    """-> (the loss of stage2_text_loss, the seg tokens it was computed from); heads: (seg_tokens, det_token) of a
    forward the caller has already run"""
    seg_tokens, det = autograd.visual_heads(adapted_model, image) if heads is None else heads
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


def stage2_loss(adapted_model, image, mask, label, anchors, img_size, iqm_queries=None):
    """The stage-2 loss (reference train.py:152-212): stage2_text_loss plus, per tap level,
        IQM_WEIGHT * SEG_LOSS_SCALE * seg_loss(iqm_map_train(seg, iqm_queries, img_size), mask)
    iqm_queries None: the queries are the IQM branch's own, from the same forward as the seg tokens and with a graph
    (autograd.visual_outputs), so backward() reaches model.iqm, class_query_mlp, query_adapters, the two feature
    projections and iqm_layer_norm as well as the image adapters.
    iqm_queries [B, 2, E] given (row 0 normal, row 1 abnormal): any tensor of that shape serves; if it requires grad it
    receives its gradient, and the seg tokens pass theirs on to seg_proj and the layer adapters.
    A query width other than the seg tokens' raises ValueError: the reference draws a fresh random nn.Linear at every
    step there (train.py:175-179), which cannot be reproduced."""
    E = adapted_model.image_adapter["seg_proj"][0].weight.shape[0]
    heads = None
    if iqm_queries is None:
        if adapted_model.iqm_hidden_size != E:
            raise ValueError(f"stage2_loss: iqm_queries must be [B, 2, {E}] (the seg tokens' width), the branch's are "
                             f"{adapted_model.iqm_hidden_size} wide")
        seg_tokens, det, iqm_queries = autograd.visual_outputs(adapted_model, image, anchors)
        heads = (seg_tokens, det)
    if iqm_queries.dim() != 3 or iqm_queries.shape[1] != 2 or iqm_queries.shape[-1] != E:
        raise ValueError(f"stage2_loss: iqm_queries must be [B, 2, {E}] (the seg tokens' width), got "
                         f"{tuple(iqm_queries.shape)}")
    loss, seg_tokens = _stage2_text_terms(adapted_model, image, mask, label, anchors, img_size, heads)
    for seg in seg_tokens:
        loss = loss + iqm_map_loss(seg, iqm_queries, mask, img_size)
    return loss


IMAGE_CHECKPOINT_NAME = "image_adapter.pth"
IQM_BRANCH_MODULES = ("iqm", "class_query_mlp", "query_adapters", "visual_feature_proj", "text_feature_proj",
                      "iqm_layer_norm")


def iqm_branch_state(adapted_model):
    """{module name: state_dict} of everything the reference's iqm_params optimizer group trains, plus the two feature
    projections and iqm_layer_norm that the branch reads."""
    return {n: getattr(adapted_model, n).state_dict() for n in IQM_BRANCH_MODULES}


def load_iqm_branch_state(adapted_model, state):
    for n in IQM_BRANCH_MODULES:
        getattr(adapted_model, n).load_state_dict(state[n], strict=True)


def train_image_adapter(model: nn.Module, text_embeddings, train_loader, optimizer: torch.optim.Optimizer, scheduler,
                        device: str, start_epoch: int, save_path: str, image_epoch: int, img_size: int,
                        logger: logging.Logger):
    """Same arguments and loop as the reference's function (train.py:117-237).  text_embeddings: {class name: anchors
    [E, 2]}; train_loader: any iterable of {"image", "mask", "label", "class_name"} batches.  Per batch: stage2_loss
    with the branch's own queries, optimizer.zero_grad(), backward, optimizer.step(), scheduler.step().
    The reference calls clip_grad_norm_ BEFORE zero_grad(), i.e. on the gradients of the previous step that zero_grad
    then discards: it never changes an update, so it is left out here.
    Checkpoint after every epoch, <save_path>/image_adapter.pth and image_adapter_<epoch + 1>.pth, with the reference's
    three keys {"epoch", "image_adapter", "image_optimizer"} plus one it lacks, "iqm_branch" (iqm_branch_state): the
    reference never saves the branch it trains, so its trained IQM weights are lost with the process."""
    for epoch in range(start_epoch, image_epoch):
        logger.info(f"training image epoch {epoch}:")
        step_losses = []
        for batch in train_loader:
            image = batch["image"].to(device)
            mask = batch["mask"].to(device)
            label = batch["label"].to(device)
            anchors = torch.stack([text_embeddings[c] for c in batch["class_name"]], dim=0)
            loss = stage2_loss(model, image, mask, label, anchors, img_size)
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            step_losses.append(loss.item())
            scheduler.step()
        logger.info(f"loss: {sum(step_losses) / len(step_losses)}")
        os.makedirs(save_path, exist_ok=True)
        state = {"epoch": epoch + 1, "image_adapter": model.image_adapter.state_dict(),
                 "image_optimizer": optimizer.state_dict(), "iqm_branch": iqm_branch_state(model)}
        torch.save(state, os.path.join(save_path, IMAGE_CHECKPOINT_NAME))
        torch.save(state, os.path.join(save_path, f"image_adapter_{epoch + 1}.pth"))
    return model
