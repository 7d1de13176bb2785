"""eval_png.py with bootstrap confidence intervals beside AUROC and AP: its arguments and steps, plus

  --bootstrap R              R bootstrap replicates per class, resampling IMAGES with replacement (a cluster bootstrap: the
                             pixels of one image are not independent).  Adds "<column> lo" / "<column> hi" for pixel AUC,
                             pixel AP, image AUC and image AP to every row and to the average: the percentile interval of
                             the replicates that hold both labels.  With --device_metrics every class costs one more sort
                             per level and the weighted curve pass of csrc/bootstrap.hip over all R replicates; without it
                             the numpy definition (forward_utils.bootstrap_eval) runs on the host, which is meant for
                             small classes.
  --bootstrap_seed S         seed of the draws (default 0); class c of the dataset draws from default_rng([S, c]), so two
                             runs over the same images -- with and without --tiles, say -- see the same replicates
  --bootstrap_level L        level of the interval (default 0.95): the quantiles (1 - L) / 2 and (1 + L) / 2
  --bootstrap_stratified     draw the normal and the anomalous images separately, each group keeping its size; a class
                             that loses more than 5 % of its replicates to a missing label is refused without it

The normalisation range and the 0.5 * max_pixel + 0.5 * image score combination are those of the whole class; they are
not recomputed per replicate.  AUPRO, F1-max and the defect columns get no interval.  With --save_path the replicates go
to <save_path>/bootstrap/<dataset>/<class>.npz (and Average.npz): pixel_auc, pixel_ap, image_auc, image_ap [R], valid [R],
seed, images, R, level, stratified and the point estimates; tools/bootstrap_diff.py reads two such trees and prints the
interval of the difference.  Under WORLD_SIZE > 1 --bootstrap is refused, like --tiles.  Without --bootstrap the script
prints and writes exactly what eval_png.py does.
evaluate(..., bootstrap=None) is the function form; write_bootstrap writes the .npz files.

python eval_bootstrap.py --save_path ... --device_metrics --bootstrap 1000 [--bootstrap_stratified] [every argument of eval_png.py]
"""
from __future__ import annotations

import argparse
import os

import numpy as np

import eval_defects as ED
import eval_last as EL
import eval_overlay as EO
import eval_png as EP
import eval_tiled as ET
from forward_utils import BOOTSTRAP_COLS, SUPPORT_WEIGHT, TILE_OVERLAP

NPZ_KEYS = {"pixel AUC": "pixel_auc", "pixel AP": "pixel_ap", "image AUC": "image_auc", "image AP": "image_ap"}


def bootstrap_settings(R, seed: int = 0, level: float = 0.95, stratified: bool = False):
    """-> the dict that evaluate(bootstrap=...) takes, or None for R = None"""
    if R is None:
        return None
    if int(R) < 1 or not 0.0 < float(level) < 1.0:
        raise ValueError("bootstrap: R must be at least 1 and the level must lie in (0, 1)")
    return {"R": int(R), "seed": int(seed), "level": float(level), "stratified": bool(stratified)}


def write_bootstrap(save_path: str, dataset: str, rows, details) -> list:
    """<save_path>/bootstrap/<dataset>/<class>.npz for every class of `details` that holds "bootstrap", and Average.npz from
    eval_last.bootstrap_average; `point` is the row's four numbers in percent.  -> the paths written"""
    folder = os.path.join(save_path, "bootstrap", dataset)
    os.makedirs(folder, exist_ok=True)
    by_name = {r["class name"]: r for r in rows}
    classes = [c for c, d in details.items() if "bootstrap" in d]
    blocks = {c: details[c]["bootstrap"] for c in classes}
    if classes:
        first = blocks[classes[0]]
        blocks["Average"] = dict(EL.bootstrap_average({}, [blocks[c] for c in classes]), seed=first["seed"], R=first["R"],
                                 level=first["level"], stratified=first["stratified"],
                                 images=sum(blocks[c]["images"] for c in classes))
    paths = []
    for name, b in blocks.items():
        paths.append(os.path.join(folder, f"{name}.npz"))
        np.savez(paths[-1], valid=np.asarray(b["valid"], bool), seed=np.int64(b["seed"]), images=np.int64(b["images"]),
                 R=np.int64(b["R"]), level=np.float64(b["level"]), stratified=np.bool_(b["stratified"]),
                 point=np.array([float(by_name[name][c]) for c in BOOTSTRAP_COLS], np.float64),
                 **{NPZ_KEYS[c]: np.asarray(b[c], np.float64) for c in BOOTSTRAP_COLS})
    return paths


def evaluate(model, image_datasets, text_embeddings, device, img_size: int, dataset: str, batch_size: int = 32,
             loader_kwargs=None, logger=None, use_iqm: bool = True, device_metrics: bool = False, aupro_limit=None,
             f1_max: bool = False, return_masks: bool = False, defects=None, save_path=None, support=None,
             support_weight: float = SUPPORT_WEIGHT, support_form=None, support_datasets=None, coreset=None,
             coreset_dim: int = 128, tiles=None, tile_overlap: int = TILE_OVERLAP, overlay=None, overlay_limit=None,
             overlay_thickness: int = 1, overlay_colormap: str = "jet", overlay_written=None, overlay_encoder: str = "pillow",
             masks_png: bool = False, masks_written=None, bootstrap=None, bootstrap_written=None):
    """eval_png.evaluate, which it is for bootstrap=None.  bootstrap: the dict of bootstrap_settings -- the interval columns
    in every row and in the average (eval_last.evaluate_rows' keyword; with tiles eval_tiled.evaluate_tiled's), the
    replicates under details[class]["bootstrap"] and, with save_path, in <save_path>/bootstrap/<dataset>/ (bootstrap_written:
    None or a list that receives the paths).  The files of overlay / masks_png are written as eval_png.evaluate writes
    them.  -> rows, or (rows, details) with return_masks.  One process only."""
    where = (model, image_datasets, text_embeddings, device, img_size, dataset)
    below = dict(batch_size=batch_size, loader_kwargs=loader_kwargs, logger=logger, use_iqm=use_iqm,
                 device_metrics=device_metrics, aupro_limit=aupro_limit, f1_max=f1_max, return_masks=return_masks,
                 defects=defects, save_path=save_path, support=support, support_weight=support_weight,
                 support_form=support_form, support_datasets=support_datasets, coreset=coreset, coreset_dim=coreset_dim)
    files = dict(overlay=overlay, overlay_limit=overlay_limit, overlay_thickness=overlay_thickness,
                 overlay_colormap=overlay_colormap, overlay_written=overlay_written, overlay_encoder=overlay_encoder,
                 masks_png=masks_png, masks_written=masks_written)
    if bootstrap is None:
        return EP.evaluate(*where, **below, tiles=tiles, tile_overlap=tile_overlap, **files)
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise ValueError("bootstrap runs in one process (the replicates of a sharded class are not gathered)")
    bootstrap = bootstrap_settings(**bootstrap)
    EP.check_encoder(overlay_encoder)
    with_files = masks_png or overlay is not None
    after = None
    if with_files:
        after = EP.files_callback(save_path, dataset, device, batch_size, loader_kwargs, defects, tiles, **files)
    f1 = f1_max or defects is not None or with_files
    if return_masks and not f1:
        raise ValueError("evaluate: return_masks needs f1_max=True (the masks are those of its threshold)")
    rows, details = ET.evaluate_details(*where, None if tiles is None else (tiles, tile_overlap),
                                        **dict(below, f1_max=f1, return_masks=return_masks or with_files),
                                        after_class=after, bootstrap=bootstrap)
    if save_path is not None:
        paths = write_bootstrap(save_path, dataset, rows, details)
        if bootstrap_written is not None:
            bootstrap_written.extend(paths)
    return EO.own_masks_only(rows, details, return_masks)


def build_parser() -> argparse.ArgumentParser:
    parser = EP.build_parser()
    parser.add_argument("--bootstrap", type=int, default=None, metavar="R",
                        help="R bootstrap replicates over the images of every class: percentile intervals beside pixel / "
                             "image AUC and AP, and the replicates under <save_path>/bootstrap/<dataset>/")
    parser.add_argument("--bootstrap_seed", type=int, default=0, help="seed of the draws; class c draws from [seed, c]")
    parser.add_argument("--bootstrap_level", type=float, default=0.95, help="level of the interval, in (0, 1)")
    parser.add_argument("--bootstrap_stratified", action="store_true",
                        help="draw the normal and the anomalous images separately, each group keeping its size")
    return parser


def _check_arguments(parser: argparse.ArgumentParser, args) -> None:
    """what the scripts below this one refuse, and this one's own"""
    if args.bootstrap < 1:
        parser.error("--bootstrap takes at least 1 replicate")
    if not 0.0 < args.bootstrap_level < 1.0:
        parser.error("--bootstrap_level takes a level in (0, 1)")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        parser.error("--bootstrap runs in one process: the replicates of a sharded class are not gathered")
    EO._check_arguments(parser, args)


def run(parser: argparse.ArgumentParser, argv=None):
    """Without --bootstrap: eval_png.run.  With it: the session of eval_png.run and this module's evaluate."""
    args = parser.parse_args(argv)
    if args.bootstrap is None:
        return EP.run(parser, argv)
    _check_arguments(parser, args)
    session, where = EO.open_session(args, __name__)
    f1 = bool(args.f1max) or args.defects is not None or args.masks_png or args.overlay is not None
    written = []
    rows = evaluate(*where, f1_max=f1, **ET.session_keywords(args, session), **EO.overlay_keywords(args),
                    overlay_encoder=args.overlay_encoder, masks_png=args.masks_png,
                    bootstrap=bootstrap_settings(args.bootstrap, args.bootstrap_seed, args.bootstrap_level,
                                                 args.bootstrap_stratified), bootstrap_written=written)
    session.logger.info("bootstrap: %d replicates, seed %d, level %s, %s; %d files", args.bootstrap, args.bootstrap_seed,
                        args.bootstrap_level, "stratified" if args.bootstrap_stratified else "plain", len(written))
    ED.log_table(session.logger, rows)
    return rows


def main(argv=None):
    return run(build_parser(), argv)


if __name__ == "__main__":
    main()
