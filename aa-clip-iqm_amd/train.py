"""Training on the HIP path end to end.

Stage 1 (reference train.py:57-113) fits the text adapters against frozen V-V ("surgery") patch features of CLIP:
encode_text forward and backward (aaclip_hip.autograd.TextTower), the train-mode similarity map and the segmentation
loss with their backward kernels.  `train_text_adapter` is fed by any iterable of {"image", "mask", "class_name"}
batches.

Stage 2 (reference train.py:117-237) fits the image adapters and the IQM branch: `stage2_loss` is the reference's loss
-- the classification term, the text-anchor maps and the IQM maps -- on one forward with a graph
(aaclip_hip.autograd.visual_outputs: tap streams, tap / det heads and the IQM branch's final queries, each with its HIP
backward), and `train_image_adapter` is the reference's epoch loop around it.

`main` is the reference's entry point (train.py:240-436) around the two loops: the same arguments and defaults, model
construction, optimisers, scheduler, resume rules and DataLoaders; `run(args)` is everything after the parser, so that
a caller can hand in its own model factory.  The train-time datasets are dataset.get_train_datasets; with
`--device_augment` their per-sample input work (colour jitter, resize, normalise, mask resize, rotation / shift /
flips) runs as HIP kernels on raw uint8 frames (aaclip_hip.engine.train_preprocess) instead of in the workers.

    python train.py --dataset MVTec --training_mode full_shot --iqm_hidden_size 768 --save_path ckpt/run [--device_augment]

(stage2_loss needs the IQM queries as wide as the seg tokens, 768 for ViT-L-14-336: see its docstring.)

The backward of the visual blocks is fp32 by default.  The environment variable AACLIP_BACKWARD selects its arithmetic
without a command-line argument (the parser stays the reference's):

    AACLIP_BACKWARD=bf16x3 python train.py --dataset MVTec --training_mode full_shot --iqm_hidden_size 768 --save_path ckpt/run

runs those blocks' products and attention backward as three-term bf16 sums on the bf16 MFMA
(aaclip_hip.autograd.backward_precision, include/aaclip.h "bf16x3"); forward outputs and loss values are the same bits
in both modes, the text tower and everything outside the visual blocks stay fp32.

The IQM branch trains in its projected form by default: query_adapters applied to every patch row of every tap level,
whatever form inference takes.  At the defaults (a 16-bit tower, no --relu) inference runs the branch's visual
cross-attention in the folded 16-bit form instead, on the LayerNorm'ed tap rows themselves, and

    AACLIP_IQM_TRAIN_FORM=folded python train.py --dataset MVTec --training_mode full_shot --iqm_hidden_size 768 --save_path ckpt/run

trains that very forward (aaclip_hip.autograd.iqm_train_form, IqmQueriesFolded; include/aaclip.h
aaclip_cross_rows_levels_backward): the queries the loss sees are the bits test_last.py evaluates.  It raises
NotImplementedError before any launch on a model whose forward does not fold (fp32, --relu, a tower neither 768 nor
1024 wide).

The optimizers are torch's.  `run` also reads two attributes that this parser never sets and train_fused.py's does:
`fused_optimizer` builds both from aaclip_hip.optim (FusedAdam / FusedAdamW: one multi-tensor HIP step, checkpoints in
torch's layout either way), and `clip_grad_norm` then clips the stage-2 step inside optimizer.step().
"""
from __future__ import annotations

import argparse
import logging
import os

import torch
from torch import nn

import forward_utils as FU
from aaclip_hip import autograd
from model.clip import create_model

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


# ------------------------------------------------------------------------------------------------ entry point
NUM_WORKERS = 4                                  # reference train.py:380
HOST_THREADS = 4                                 # reference train.py:27-34


# name -> (default, help): the reference's command line (train.py:241-284); types follow the defaults
ARGUMENTS = {
    "model_name": ("ViT-L-14-336", "model config under model/model_configs"),
    "img_size": (518, "side of the square input image"),
    "surgery_until_layer": (20, "stage 1: V-V attention from this visual block on"),
    "dataset": ("VisA", "training dataset, a key of dataset.constants.DATA_PATH"),
    "shot": (32, "samples per class of the few-shot metadata file"),
    "text_batch_size": (16, "stage 1 batch"),
    "image_batch_size": (2, "stage 2 batch"),
    "text_epoch": (5, "stage 1 epochs"),
    "image_epoch": (20, "stage 2 epochs"),
    "text_lr": (0.00001, "stage 1 learning rate"),
    "image_lr": (0.0005, "stage 2 learning rate (the IQM group runs at a tenth)"),
    "seed": (111, None),
    "save_path": ("ckpt/baseline", "checkpoints and train.log; an existing directory is resumed"),
    "text_norm_weight": (0.1, "weight of the anchor-overlap term of stage 1"),
    "text_adapt_weight": (0.1, None),
    "image_adapt_weight": (0.1, None),
    "text_adapt_until": (3, "text blocks with an adapter"),
    "image_adapt_until": (6, "visual blocks with an adapter"),
    "iqm_hidden_size": (512, "width of the IQM branch; stage2_loss needs the seg tokens' width"),
    "iqm_num_layers": (2, None),
    "iqm_num_heads": (8, None),
    "iqm_weight": (0.4, "accepted like the reference does, which never reads it (IQM_WEIGHT is fixed)"),
}


def build_parser() -> argparse.ArgumentParser:
    """The reference's arguments and defaults plus --device_augment."""
    parser = argparse.ArgumentParser(description="Training")
    for name, (default, text) in ARGUMENTS.items():
        parser.add_argument("--" + name, type=type(default), default=default, help=text)
    parser.add_argument("--relu", action="store_true", help="ReLU instead of LeakyReLU behind the projections")
    parser.add_argument("--training_mode", type=str, default="few_shot", choices=["few_shot", "full_shot"])
    parser.add_argument("--criterion", type=str, default=["dice_loss", "focal_loss"], nargs="+",
                        help="accepted like the reference does, which never reads it")
    parser.add_argument("--device_augment", action="store_true",
                        help="colour jitter, resize, normalise and the geometric augmentation on the GPU")
    return parser


def _loader(dataset, batch_size, device, device_augment):
    from torch.utils.data import DataLoader

    import dataset as D
    kwargs = {"num_workers": NUM_WORKERS, "pin_memory": True} if device.type == "cuda" else {}
    if not device_augment:
        return DataLoader(dataset, batch_size=batch_size, shuffle=True, **kwargs)
    return D.DeviceAugmentLoader(DataLoader(dataset, batch_size=batch_size, shuffle=True, collate_fn=D.collate_raw,
                                            **kwargs), device)


def run(args, model_factory=create_model, levels=(6, 12, 18, 24)):
    """Everything of the reference's main() after the parser (train.py:287-436).  model_factory: called twice with
    create_model's keywords (model_name, img_size, device, pretrained="openai", require_pretrained=True) -> a CLIP;
    levels: the tap levels, which the reference hard-codes.  Returns the trained model."""
    import dataset as D
    from model.adapter import AdaptedCLIP
    from utils import setup_seed

    setup_seed(args.seed)
    os.makedirs(args.save_path, exist_ok=True)
    logger = logging.getLogger(__name__)
    logging.basicConfig(filename=os.path.join(args.save_path, "train.log"), encoding="utf-8", level=logging.INFO)
    logger.info("args: %s", vars(args))
    use_cuda = torch.cuda.is_available()
    device = torch.device("cuda:0" if use_cuda else "cpu")
    levels = list(levels)
    # the frozen image side of stage 1: CLIP after "surgery"
    clip_surgery = model_factory(model_name=args.model_name, img_size=args.img_size, device=device, pretrained="openai",
                                 require_pretrained=True)
    clip_surgery.eval()
    clip_surgery.visual.DAPM_replace(DPAM_layer=args.surgery_until_layer)
    clip_model = model_factory(model_name=args.model_name, img_size=args.img_size, device=device, pretrained="openai",
                               require_pretrained=True)
    clip_model.eval()
    model = AdaptedCLIP(clip_model=clip_model, text_adapt_weight=args.text_adapt_weight,
                        image_adapt_weight=args.image_adapt_weight, text_adapt_until=args.text_adapt_until,
                        image_adapt_until=args.image_adapt_until, levels=levels, relu=args.relu,
                        iqm_hidden_size=args.iqm_hidden_size, iqm_num_layers=args.iqm_num_layers,
                        iqm_num_heads=args.iqm_num_heads).to(device)
    model.eval()
    # only what an optimizer below steps asks for a gradient
    image_params = list(model.image_adapter.parameters())
    iqm_params = (list(model.iqm.parameters()) + list(model.class_query_mlp.parameters())
                  + list(model.query_adapters.parameters()))
    for p in list(model.parameters()) + list(clip_surgery.parameters()):
        p.requires_grad_(False)
    for p in list(model.text_adapter.parameters()) + image_params + iqm_params:
        p.requires_grad_(True)
    adam, adamw, clip = torch.optim.Adam, torch.optim.AdamW, {}
    if getattr(args, "fused_optimizer", False):          # train_fused.py; the state and checkpoints keep torch's layout
        from aaclip_hip import optim
        adam, adamw = optim.FusedAdam, optim.FusedAdamW
        # the reference clips in stage 2 alone (train.py:214, on gradients it then discards); here inside step()
        clip = {"max_grad_norm": getattr(args, "clip_grad_norm", None)}
    elif getattr(args, "clip_grad_norm", None) is not None:
        raise ValueError("train.run: clip_grad_norm needs fused_optimizer (the clipping lives inside its step())")
    text_optimizer = adam(model.text_adapter.parameters(), lr=args.text_lr, betas=(0.5, 0.999))
    image_optimizer = adamw([{"params": image_params, "lr": args.image_lr, "weight_decay": 1e-4},
                             {"params": iqm_params, "lr": args.image_lr * 0.1, "weight_decay": 1e-3}],
                            betas=(0.9, 0.999), **clip)
    image_scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(image_optimizer, T_max=args.image_epoch, eta_min=1e-6)
    # resume (train.py:356-375)
    text_start_epoch = 0
    text_file = os.path.join(args.save_path, CHECKPOINT_NAME)
    if os.path.exists(text_file):
        checkpoint = torch.load(text_file, map_location=device)
        model.text_adapter.load_state_dict(checkpoint["text_adapter"])
        text_optimizer.load_state_dict(checkpoint["text_optimizer"])
        text_start_epoch = checkpoint["epoch"]
        adapt_text = not (text_start_epoch == (args.text_epoch - 1))
    else:
        adapt_text = args.text_epoch != 0
    image_start_epoch = 0
    image_file = os.path.join(args.save_path, IMAGE_CHECKPOINT_NAME)
    if os.path.exists(image_file):
        checkpoint = torch.load(image_file, map_location=device)
        image_start_epoch = checkpoint["epoch"]
        model.image_adapter.load_state_dict(checkpoint["image_adapter"])
        image_optimizer.load_state_dict(checkpoint["image_optimizer"])
        if "iqm_branch" in checkpoint:           # the reference never saves the branch it trains
            load_iqm_branch_state(model, checkpoint["iqm_branch"])
    # datasets
    if args.training_mode == "full_shot":
        args.shot = -1
    logger.info("loading dataset ...")
    text_dataset, image_dataset = D.get_train_datasets(args.dataset, args.img_size, args.training_mode, args.shot, logger,
                                                       device_augment=args.device_augment)
    text_dataloader = _loader(text_dataset, args.text_batch_size, device, args.device_augment)
    logger.info("loading image adaptation dataset ...")
    image_dataloader = _loader(image_dataset, args.image_batch_size, device, args.device_augment)
    # training
    if adapt_text:
        model = train_text_adapter(adapted_model=model, clip_surgery=clip_surgery, text_norm_weight=args.text_norm_weight,
                                   train_loader=text_dataloader, optimizer=text_optimizer, device=device,
                                   start_epoch=text_start_epoch, dataset_name=args.dataset, save_path=args.save_path,
                                   text_epoch=args.text_epoch, img_size=args.img_size, logger=logger, levels=levels)
    del text_dataloader, text_dataset, clip_surgery, text_optimizer
    if use_cuda:
        torch.cuda.empty_cache()
    with torch.no_grad():
        text_embeddings = FU.get_adapted_text_embedding(clip_model if args.text_epoch == 0 else model, args.dataset,
                                                        device)
    return train_image_adapter(model=model, text_embeddings=text_embeddings, image_epoch=args.image_epoch,
                               train_loader=image_dataloader, optimizer=image_optimizer, scheduler=image_scheduler,
                               device=device, start_epoch=image_start_epoch, save_path=args.save_path,
                               img_size=args.img_size, logger=logger)


def host_threads():
    """the reference's thread settings (train.py:27-34)"""
    for name in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS", "VECLIB_MAXIMUM_THREADS",
                 "NUMEXPR_NUM_THREADS"):
        os.environ[name] = str(HOST_THREADS)
    torch.set_num_threads(HOST_THREADS)
    os.environ["TOKENIZERS_PARALLELISM"] = "false"


def main(argv=None):
    args = build_parser().parse_args(argv)
    host_threads()
    return run(args)


if __name__ == "__main__":
    main()
