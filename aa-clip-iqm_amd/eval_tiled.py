"""eval_coreset.py at more than the model's 518 x 518 pixels: its arguments and steps, plus

  --tiles G          evaluate every frame at C x C pixels, C = S + (G - 1) * (S - O) with S = --img_size, as G x G
                     overlapping tiles of the model's size: the frame is resized to C (not to S), cut into tiles on the
                     GPU (csrc/tiles.hip, a copy of bits), every tile goes through the model and the map steps at size S,
                     and the G * G tile maps are blended back into one C x C map on the GPU -- a pixel under one tile
                     keeps that tile's value, a pixel in an overlap is the weighted mean of its 2 or 4 tiles with the
                     weights min(y + 1, S - y) * min(x + 1, S - x), a linear cross-fade.  The image score of a frame is
                     the MAXIMUM of its tiles' scores: an anomaly lies in some tile, and the tiles without it must not
                     average it away.  Masks and metrics are those of the C x C frame.  --tiles 2 is 924 x 924 and
                     --tiles 3 is 1330 x 1330 at the defaults.  Image batches hold max(1, image_batch_size // G^2) frames,
                     so a tile batch is about --image_batch_size.
  --tile_overlap O   default 112 = 8 grid cells of 14 px, 0 <= O <= S // 2.  Derived, not tuned (no dataset was at hand): a
                     tile's map is blurred over at most 9 cells, a radius of 4 cells = 56 px, with a reflected border; in
                     an overlap of 112 px the half of the cross-fade where a tile's blur saw reflected cells carries less
                     than half the weight.

With --support K the bank of a class is built from the TILES of its K support frames (K * G^2 * P rows per level, before
--support_coreset), so a test tile is compared with good tiles of every position.  Without --tiles it prints exactly what
eval_coreset.py prints.  Under WORLD_SIZE > 1 --tiles is refused: sharded tiled evaluation is not part of this script.
evaluate(..., tiles=G, tile_overlap=O) is the function form, on datasets built at C.

python eval_tiled.py --save_path ... [--tiles G] [--tile_overlap O] [every argument of eval_coreset.py]
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

import eval_coreset as EC
import eval_defects as ED
import eval_last as EL
import eval_support as ES
import test_last as TL
from aaclip_hip import engine
from dataset import DOMAINS
from forward_utils import (DEFECT_COLS, SUPPORT_WEIGHT, TILE_OVERLAP, build_support_bank, calculate_anomaly_map, image_score,
                           metrics_eval, metrics_eval_device, support_anomaly_map, tile_origins)


def tile_geometry(img_size: int, tiles: int, tile_overlap: int):
    """-> (S, G, O, C) for the model's side, the tiles per side and the overlap; ValueError for a geometry the kernels
    refuse (forward_utils.tile_origins states the rule)"""
    S, G, O = int(img_size), int(tiles), int(tile_overlap)
    tile_origins(S, G, O)
    return S, G, O, S + (G - 1) * (S - O)


def frames_per_batch(batch_size: int, tiles) -> int:
    """the frames in a loader batch: batch_size, or with tiles=G as many as give about batch_size tiles"""
    return batch_size if tiles is None else max(1, batch_size // (int(tiles) ** 2))


def _canvas_batch(input_data, device, S, G, O, C):
    """one loader batch -> its normalised frames [b, 3, C, C] on the device; a frame or mask of another size is an error"""
    image = input_data["image"].to(device, non_blocking=True)
    if image.dtype == torch.uint8:                       # raw HWC frames: resize to the CANVAS + normalise on the GPU
        image = engine.preprocess(image, C)
    if tuple(image.shape[-2:]) != (C, C):
        raise ValueError(f"tiled evaluation: {G} x {G} tiles of {S} px with {O} px of overlap need frames of {C} x {C} px "
                         f"(datasets built at img_size = {C}), got {tuple(image.shape)}")
    return image.float().contiguous()


def get_predictions_tiled(model, class_text_embeddings: torch.Tensor, test_loader, device, img_size: int,
                          dataset: str = "MVTec", use_iqm: bool = True, on_device: bool = False, tiles=(1, 0), support=None,
                          support_weight: float = SUPPORT_WEIGHT):
    """eval_last.get_predictions_support for frames of C x C pixels seen as tiles=(G, O): G x G tiles of img_size (the
    model's side S) that overlap by O pixels, C = S + (G - 1) * (S - O).  The loader's dataset is built at C, so images
    and masks arrive at canvas size (uint8 frames go through engine.preprocess(image, C)).  Per batch: engine.tile_gather,
    then the per-batch steps of get_predictions / get_predictions_support on the tile batch at size S (the model,
    image_score, calculate_anomaly_map, the support term when `support` is an engine.SupportBank -- built from tiles, see
    evaluate -- and the IQM fusion), then engine.tile_stitch of the final tile maps and the maximum of a frame's tile
    scores.  -> get_predictions' tuple with maps [N, C, C] and masks [N, 1, C, C]; on_device as there.  tiles=(1, 0) is
    get_predictions_support bit for bit.  The indices of the nearest bank rows are not collected."""
    G, O = tiles
    S, G, O, C = tile_geometry(img_size, G, O)
    masks, labels, preds, preds_image, file_names = [], [], [], [], []
    domain = DOMAINS[dataset]
    for input_data in test_loader:
        assert len(set(input_data["class_name"])) == 1, "mixed class not supported"
        if tuple(input_data["mask"].shape[-2:]) != (C, C):
            raise ValueError(f"tiled evaluation: masks of {tuple(input_data['mask'].shape[-2:])} px, but {G} x {G} tiles "
                             f"of {S} px with {O} px of overlap need datasets built at img_size = {C}")
        image = _canvas_batch(input_data, device, S, G, O, C)
        if on_device:
            masks.append((input_data["mask"].to(device, non_blocking=True) != 0).to(torch.uint8))
        else:
            masks.append(np.asarray(input_data["mask"].cpu().numpy()))
        labels.append(np.asarray(torch.as_tensor(input_data["label"]).cpu().numpy()))
        file_names.extend(input_data["file_name"])
        frames = image.size(0)
        tile_batch = engine.tile_gather(image, S, G, O)
        epoch_text_feature = class_text_embeddings.unsqueeze(0).repeat(tile_batch.size(0), 1, 1) if use_iqm else None
        patch_features, det_feature, iqm_outputs = model(tile_batch, text_embeddings=epoch_text_feature)
        score = image_score(det_feature, class_text_embeddings).float().reshape(frames, G * G).max(dim=1).values
        tile_map = calculate_anomaly_map(patch_features, class_text_embeddings, S, domain=domain)
        if support is not None:
            tile_map = support_anomaly_map(patch_features, support, S, domain=domain, base=tile_map, weight=support_weight)
        if iqm_outputs is not None:
            tile_map = engine.iqm_map(patch_features, iqm_outputs.last_hidden_state, S, base=tile_map,
                                      w_base=TL.TEXT_WEIGHT, w_iqm=TL.IQM_WEIGHT)
        final_map = engine.tile_stitch(tile_map.contiguous(), G, O, frames)
        preds_image.append(score if on_device else score.cpu().numpy())
        preds.append(final_map if on_device else final_map.cpu().numpy())
    cat = (lambda v: torch.cat(v, dim=0)) if on_device else (lambda v: np.concatenate(v, axis=0))
    return cat(masks), np.concatenate(labels, axis=0), cat(preds), cat(preds_image), file_names


def tiled_support_banks(model, image_datasets, k: int, device, img_size: int, tiles, form=None, support_datasets=None,
                        batch_size: int = 32, coreset=None, coreset_dim: int = 128):
    """eval_last.support_banks for datasets built at the canvas size: the bank of a class holds the seg tokens of the
    G * G tiles of each of its k support frames, k * G^2 * P rows per level in (frame, tile, patch) order
    (forward_utils.build_support_bank on tile batches; coreset as there).  -> (banks, evaluated datasets)."""
    G, O = tiles
    S, G, O, C = tile_geometry(img_size, G, O)
    banks, evaluated = {}, {}
    for class_name, ds in image_datasets.items():
        if support_datasets is None:
            shots, evaluated[class_name] = ds.support_split(k)
        else:
            shots, evaluated[class_name] = support_datasets[class_name].support_split(k)[0], ds
        batches = []
        for b in torch.utils.data.DataLoader(shots, batch_size=frames_per_batch(batch_size, G), shuffle=False):
            batches.append(engine.tile_gather(_canvas_batch(b, device, S, G, O, C), S, G, O))
        extra = {} if coreset is None else {"coreset": coreset, "coreset_dim": coreset_dim}
        banks[class_name] = build_support_bank(model, batches, form, **extra)
    return banks, evaluated


def evaluate_tiled(model, image_datasets, text_embeddings, device, img_size: int, dataset: str, tiles, batch_size: int = 32,
                   loader_kwargs=None, logger=None, use_iqm: bool = True, device_metrics: bool = False, fpr_limit=None,
                   f1_max: bool = False, return_masks: bool = False, defects=None, support=None,
                   support_weight: float = SUPPORT_WEIGHT, bootstrap=None, after_class=None):
    """The per-class loop of eval_last.evaluate_rows over get_predictions_tiled, in one process: -> (rows, details), details
    None without f1_max and without bootstrap (evaluate_rows' keyword, passed to every class and to the average).  tiles=(G, O); support: None or {class name: bank of tiled_support_banks}; the other keywords are
    evaluate_rows', after_class included (its frames, masks and maps are C x C).  The maps handed to metrics_eval /
    metrics_eval_device are C x C."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise ValueError("tiled evaluation runs in one process (sharded tiled evaluation is not part of it)")
    if defects is not None and not f1_max:
        raise ValueError("evaluate_tiled: defects needs f1_max=True (the regions are those at the pixel F1-max threshold)")
    G, O = tiles
    S, G, O, C = tile_geometry(img_size, G, O)
    rows, details = [], {} if f1_max or bootstrap is not None else None
    row_of = metrics_eval_device if device_metrics else metrics_eval
    for class_name, image_dataset in image_datasets.items():
        loader = torch.utils.data.DataLoader(image_dataset, batch_size=frames_per_batch(batch_size, G), shuffle=False,
                                             **(loader_kwargs or {}))
        with torch.no_grad():
            masks, labels, preds, preds_image, file_names = get_predictions_tiled(
                model, text_embeddings[class_name], loader, device, S, dataset, use_iqm, device_metrics, tiles=(G, O),
                support=None if support is None else support[class_name], support_weight=support_weight)
        extra = {}
        if f1_max:
            extra["f1_max"] = True
            if defects is not None:
                extra["defects"] = defects
            scores = preds_image.detach().cpu().numpy() if torch.is_tensor(preds_image) else np.asarray(preds_image)
            extra["details"] = details[class_name] = {
                "masks": bool(return_masks), "file_names": list(file_names),
                "labels": [int(v) for v in np.asarray(labels).reshape(-1)],
                "image scores": [float(v) for v in scores.reshape(-1)]}
        if bootstrap is not None:
            extra["bootstrap"] = dict(bootstrap, class_index=len(rows))
            extra.setdefault("details", details.setdefault(class_name, {}))
        rows.append(row_of(masks, labels, preds, preds_image, class_name, domain=DOMAINS[dataset], fpr_limit=fpr_limit,
                           **extra))
        if after_class is not None:
            after_class(class_name, image_dataset, masks, labels, preds, preds_image, file_names, extra.get("details"))
        del masks, preds, preds_image          # released before the next class is evaluated
        if logger:
            logger.info("%s", rows[-1])
    cols = (TL.NUMERIC_COLS + ([EL.AUPRO_COL] if fpr_limit is not None else []) + (EL.F1_COLS if f1_max else []) +
            (DEFECT_COLS if defects is not None else []))
    avg = {c: float(np.mean([r[c] for r in rows])) for c in cols}
    avg["class name"] = "Average"
    if bootstrap is not None:
        EL.bootstrap_average(avg, [details[r["class name"]]["bootstrap"] for r in rows])
    rows.append(avg)
    return rows, details


def evaluate(model, image_datasets, text_embeddings, device, img_size: int, dataset: str, batch_size: int = 32,
             loader_kwargs=None, logger=None, use_iqm: bool = True, device_metrics: bool = False, aupro_limit=None,
             f1_max: bool = False, return_masks: bool = False, defects=None, save_path=None, support=None,
             support_weight: float = SUPPORT_WEIGHT, support_form=None, support_datasets=None, coreset=None,
             coreset_dim: int = 128, tiles=None, tile_overlap: int = TILE_OVERLAP):
    """eval_coreset.evaluate; tiles: None, which is eval_coreset.evaluate and nothing else, or G: every frame is evaluated
    at C x C pixels, C = img_size + (G - 1) * (img_size - tile_overlap), as G x G tiles of the model's img_size
    (get_predictions_tiled).  The datasets (and support_datasets) must be built at img_size = C: a dataset or a mask of
    another size raises a ValueError that names C.  Image batches hold max(1, batch_size // G^2) frames.  support=K builds
    every class's bank from the tiles of its K support frames (tiled_support_banks: K * G^2 * P rows per level, reduced by
    coreset as in eval_coreset).  With tiles, details[class]["support nearest"] is NOT produced; the other entries of
    details, the rows and the return value are eval_coreset.evaluate's."""
    where = (model, image_datasets, text_embeddings, device, img_size, dataset)
    below = dict(batch_size=batch_size, loader_kwargs=loader_kwargs, logger=logger, use_iqm=use_iqm,
                 device_metrics=device_metrics, aupro_limit=aupro_limit, f1_max=f1_max, return_masks=return_masks,
                 defects=defects, save_path=save_path, support=support, support_weight=support_weight,
                 support_form=support_form, support_datasets=support_datasets, coreset=coreset, coreset_dim=coreset_dim)
    if tiles is None:
        return EC.evaluate(*where, **below)
    f1 = f1_max or defects is not None
    if return_masks and not f1:
        raise ValueError("evaluate: return_masks needs f1_max=True (the masks are those of its threshold)")
    rows, details = evaluate_details(*where, (tiles, tile_overlap), **dict(below, f1_max=f1))
    return (rows, details) if return_masks and f1 else rows


def evaluate_details(model, image_datasets, text_embeddings, device, img_size: int, dataset: str, tiles, batch_size: int = 32,
                     loader_kwargs=None, logger=None, use_iqm: bool = True, device_metrics: bool = False, aupro_limit=None,
                     f1_max: bool = False, return_masks: bool = False, defects=None, save_path=None, support=None,
                     support_weight: float = SUPPORT_WEIGHT, support_form=None, support_datasets=None, coreset=None,
                     coreset_dim: int = 128, bootstrap=None, after_class=None):
    """The evaluation behind evaluate and the scripts above this one.  tiles=None: eval_defects.evaluate_details, the path
    at the model's own size.  tiles=(G, O), its tiled twin: the banks where support=K asks for them, evaluate_tiled
    (after_class and bootstrap are its keywords), and the .jsonl files of eval_defects.write_defects where defects and
    save_path ask for them.  -> (rows, details)."""
    if tiles is None:
        return ED.evaluate_details(model, image_datasets, text_embeddings, device, img_size, dataset, batch_size=batch_size,
                                   loader_kwargs=loader_kwargs, logger=logger, use_iqm=use_iqm,
                                   device_metrics=device_metrics, aupro_limit=aupro_limit, f1_max=f1_max,
                                   return_masks=return_masks, defects=defects, save_path=save_path, support=support,
                                   support_weight=support_weight, support_form=support_form,
                                   support_datasets=support_datasets, coreset=coreset, coreset_dim=coreset_dim,
                                   bootstrap=bootstrap, after_class=after_class)
    S, G, O, C = tile_geometry(img_size, *tiles)
    if coreset is not None and support is None:
        raise ValueError("evaluate: coreset needs support=K")
    for class_name, ds in list(image_datasets.items()) + list((support_datasets or {}).items()):
        if getattr(ds, "img_size", C) != C:
            raise ValueError(f"tiled evaluation: the dataset of {class_name} is built at img_size = {ds.img_size}, but {G} x "
                             f"{G} tiles of {S} px with {O} px of overlap need img_size = {C}")
    banks = None
    if support is not None:
        banks, image_datasets = tiled_support_banks(model, image_datasets, support, device, S, (G, O), form=support_form,
                                                    support_datasets=support_datasets, batch_size=batch_size,
                                                    coreset=coreset, coreset_dim=coreset_dim)
        if logger:
            logger.info("support banks: %d shots of %d tiles per class, form %s, weight %s", support, G * G,
                        "fp16" if next(iter(banks.values())).form == engine.SUPPORT_FP16 else "fp32", support_weight)
            if coreset is not None:
                EL.log_coreset(logger, banks)
    rows, details = evaluate_tiled(model, image_datasets, text_embeddings, device, S, dataset, (G, O), batch_size=batch_size,
                                   loader_kwargs=loader_kwargs, logger=logger, use_iqm=use_iqm,
                                   device_metrics=device_metrics, fpr_limit=aupro_limit, f1_max=f1_max,
                                   return_masks=return_masks, defects=defects, support=banks, support_weight=support_weight,
                                   after_class=after_class, bootstrap=bootstrap)
    ED.write_defects_of(defects, save_path, dataset, details)
    return rows, details


def build_parser() -> argparse.ArgumentParser:
    parser = EC.build_parser()
    parser.add_argument("--tiles", type=int, default=None, metavar="G",
                        help="evaluate at C x C pixels, C = S + (G - 1) * (S - O), as G x G overlapping tiles of --img_size")
    parser.add_argument("--tile_overlap", type=int, default=TILE_OVERLAP, metavar="O",
                        help="overlap of neighbouring tiles in pixels, 0 .. img_size // 2 (derived default 112, not tuned)")
    return parser


def _check_arguments(parser: argparse.ArgumentParser, args) -> None:
    """this script's checks where --tiles is given, then those of every script below it, for the scripts whose run()
    does not go through theirs"""
    if args.tiles is not None:
        if args.tiles < 1:
            parser.error("--tiles takes at least 1 tile per side")
        if not 0 <= args.tile_overlap <= args.img_size // 2:
            parser.error("--tile_overlap takes 0 .. img_size // 2 pixels")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            parser.error("--tiles runs in one process: sharded tiled evaluation is not part of this script")
    EL.check_arguments(parser, args)
    ED.check_arguments(parser, args)
    if args.support is None and (args.support_meta is not None or args.support_coreset is not None):
        parser.error("--support_meta and --support_coreset need --support K")
    ES.check_arguments(parser, args)
    EC.check_arguments(parser, args)


def session_keywords(args, session) -> dict:
    """the keywords of eval_coreset.evaluate that the command line and the session set: all but f1_max and return_masks"""
    return dict(batch_size=args.image_batch_size, loader_kwargs={"num_workers": 4, "pin_memory": True},
                logger=session.logger, use_iqm=args.iqm == "on", device_metrics=args.device_metrics,
                aupro_limit=args.aupro, defects=args.defects, save_path=args.save_path, support=args.support,
                support_weight=args.support_weight, support_form=args.support_form,
                support_datasets=session.support_datasets, coreset=args.support_coreset,
                coreset_dim=args.support_coreset_dim)


def run(parser: argparse.ArgumentParser, argv=None):
    """Without --tiles: eval_coreset.run.  With it: eval_last.open_session with the datasets built at the canvas size (the
    model stays at --img_size) and evaluate_details."""
    args = parser.parse_args(argv)
    if args.tiles is None:
        return EC.run(parser, argv)
    _check_arguments(parser, args)
    S, G, O, C = tile_geometry(args.img_size, args.tiles, args.tile_overlap)
    session = EL.open_session(args, __name__, C, ["tiled inference: S %d, G %d, O %d, C %d (%d tiles per frame)"
                                                  % (S, G, O, C, G * G)])
    f1 = bool(args.f1max) or args.defects is not None
    rows, details = evaluate_details(session.model, session.image_datasets, session.text_embeddings, session.device, S,
                                     args.dataset, (G, O), f1_max=f1, **session_keywords(args, session))
    if f1:
        for name, d in details.items():
            session.logger.info("%s: pixel threshold %.9g, image threshold %s (normalised units)", name,
                                d["pixel threshold"], d["image threshold"])
    ED.log_table(session.logger, rows)
    return rows


def main(argv=None):
    return run(build_parser(), argv)


if __name__ == "__main__":
    main()
