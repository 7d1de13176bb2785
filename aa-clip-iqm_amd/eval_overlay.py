"""eval_tiled.py with pictures: its arguments and steps, plus

  --overlay [ALPHA]          after every class is evaluated, render its frames on the GPU (csrc/overlay.hip, one launch per
                             batch) and write <save_path>/overlays/<dataset>/<class>/<name>.png: the frame the model saw,
                             the heat map blended over it (ALPHA, default 0.5, is the frame's weight) and the ground truth
                             blended over it, stacked vertically, with the contour of the predicted mask on the two lower
                             panels.  The predicted mask is the one at the class's pixel F1-max threshold, so --overlay
                             implies --f1max; with --defects it is the mask that the area filter kept.  <name> is the last
                             two components of the image's file name joined by "_", the extension replaced.  The heat map
                             is quantised against the class's range (engine.metrics_range of the class's maps), the way
                             the metrics normalise it.  With --tiles the frames and maps are C x C.
  --overlay_limit N          only the first N images of each class, in file order (default: all)
  --overlay_thickness T      reach of the contours in pixels, 0 .. 8 (default 1; 0 draws none)
  --overlay_colormap NAME    jet (default) or gray: engine.overlay_lut's integer tables

The definition of every byte is forward_utils.render_overlays_host.  The pass walks the evaluated dataset a second time
in file order (the loaders do not shuffle, so the order is that of the maps), holds one batch of panels at a time and
hands them to at most 8 threads that encode the PNGs with Pillow.  Under WORLD_SIZE > 1 --overlay is refused, like
--tiles.  Without --overlay the script prints exactly what eval_tiled.py prints and writes nothing more.
evaluate(..., overlay=ALPHA, ...) is the function form; write_overlays is the pass over one class.

python eval_overlay.py --save_path ... [--overlay [ALPHA]] [--overlay_limit N] [every argument of eval_tiled.py]
"""
from __future__ import annotations

import argparse
import concurrent.futures
import os

import numpy as np
import torch

import eval_defects as ED
import eval_last as EL
import eval_tiled as ET
from aaclip_hip import engine
from forward_utils import SUPPORT_WEIGHT, TILE_OVERLAP, render_overlays

OVERLAY_ALPHA = 0.5
OVERLAY_WRITERS = 8


def overlay_name(file_name: str) -> str:
    """the last two components of an image's file name joined by "_", the extension replaced by .png"""
    parts = [p for p in str(file_name).replace("\\", "/").split("/") if p]
    return os.path.splitext("_".join(parts[-2:]))[0] + ".png"


def overlay_paths(folder: str, file_names) -> list:
    """-> the path of every image's overlay; two images with one name are a ValueError"""
    names = [overlay_name(f) for f in file_names]
    seen = {}
    for name, file_name in zip(names, file_names):
        if name in seen:
            raise ValueError(f"overlays: {seen[name]} and {file_name} would both be written to {name}")
        seen[name] = file_name
    return [os.path.join(folder, name) for name in names]


def _save_png(path: str, panels: np.ndarray) -> None:
    from PIL import Image
    Image.fromarray(panels, "RGB").save(path, format="PNG")


def _range_record(preds, device) -> torch.Tensor:
    """the class's range record on the device: engine.metrics_range of device maps; for host maps their fp32 minimum and
    maximum in the record's layout (min | max as two fp32 in the first of three int64 words)"""
    if torch.is_tensor(preds):
        return engine.metrics_range(preds)[0]
    record = np.zeros(3, np.int64)
    record[:1].view(np.float32)[:] = (np.float32(preds.min()), np.float32(preds.max()))
    return torch.from_numpy(record).to(device)


def _submit_pillow(pool, panels: torch.Tensor, paths) -> list:
    """one batch of rendered panels -> the futures of its files: the panels come to the host, the pool's threads encode"""
    host = panels.cpu().numpy()
    return [pool.submit(_save_png, path, host[i]) for i, path in enumerate(paths)]


def write_overlays(folder: str, image_dataset, masks, preds, file_names, pred_masks, device, alpha: float = OVERLAY_ALPHA,
                   limit=None, thickness: int = 1, colormap: str = "jet", batch_size: int = 32, loader_kwargs=None) -> list:
    """The overlay pass over one evaluated class: `image_dataset` is walked again in file order, every batch of frames is
    brought to the device (uint8 frames through engine.preprocess to the maps' side), rendered against the class's range
    record with the predicted masks `pred_masks` and the ground truth `masks` (forward_utils.render_overlays: frame, heat
    and truth panels), and written as PNGs under `folder` by at most 8 threads.  masks [N, 1, H, W] or [N, H, W], preds
    [N, H, W], pred_masks [N, H, W] or None: device tensors (the device metrics path) or host arrays, which are uploaded
    batch by batch.  limit: None or the number of leading images.  One batch of panels is held at a time.
    -> the paths written, in file order."""
    return _overlay_pass(_submit_pillow, folder, image_dataset, masks, preds, file_names, pred_masks, device, alpha, limit,
                         thickness, colormap, batch_size, loader_kwargs)


def _overlay_pass(submit, folder: str, image_dataset, masks, preds, file_names, pred_masks, device, alpha, limit, thickness,
                  colormap, batch_size, loader_kwargs) -> list:
    """write_overlays, with submit(pool, panels, paths) -> futures as the step that turns a rendered batch into files"""
    n = len(file_names) if limit is None else max(0, min(int(limit), len(file_names)))
    if len(image_dataset) != len(file_names) or len(preds) != len(file_names):
        raise ValueError(f"overlays: {len(image_dataset)} images, {len(preds)} maps and {len(file_names)} file names")
    paths = overlay_paths(folder, list(file_names)[:n])          # before anything is written
    if n == 0:
        return paths
    H, W = (int(v) for v in preds.shape[-2:])
    record = _range_record(preds, device)
    to_device = lambda a, dtype: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(device).to(dtype)
    os.makedirs(folder, exist_ok=True)
    loader = torch.utils.data.DataLoader(image_dataset, batch_size=batch_size, shuffle=False, **(loader_kwargs or {}))
    done, pending = 0, []
    with concurrent.futures.ThreadPoolExecutor(max_workers=OVERLAY_WRITERS) as pool:
        for batch in loader:
            if done >= n:
                break
            if list(batch["file_name"]) != list(file_names[done:done + len(batch["file_name"])]):
                raise ValueError("overlays: the dataset's second walk does not give the file order of the maps")
            b = min(len(batch["file_name"]), n - done)
            image = batch["image"][:b].to(device, non_blocking=True)
            if image.dtype == torch.uint8:                       # raw HWC frames: resize to the maps' side + normalise
                if H != W:
                    raise ValueError(f"overlays: raw frames need square maps, got {H} x {W}")
                image = engine.preprocess(image, H)
            if tuple(image.shape[-2:]) != (H, W):
                raise ValueError(f"overlays: frames of {tuple(image.shape[-2:])} px for maps of {H} x {W} px")
            rows = slice(done, done + b)
            truth = (to_device(masks[rows], torch.float32).reshape(b, H, W) != 0).to(torch.uint8).contiguous()
            pred = None if pred_masks is None else to_device(pred_masks[rows], torch.uint8).reshape(b, H, W).contiguous()
            panels = render_overlays(image.float().contiguous(), to_device(preds[rows], torch.float32).contiguous(), record,
                                     pred, truth, lut=colormap, alpha256=int(round(float(alpha) * 256)), thickness=thickness)
            for f in pending:                                    # the batch before this one is on disk: one batch is held
                f.result()
            pending = submit(pool, panels, paths[done:done + b])
            done += b
        for f in pending:
            f.result()
    if done != n:
        raise ValueError(f"overlays: the dataset gave {done} of {n} images")
    return paths


def mask_callback(what: str, defects, *passes):
    """-> the after_class callable of eval_last.evaluate_rows / eval_tiled.evaluate_tiled that hands the class's predicted
    masks -- details["kept masks"] with defects, else details["masks"] -- to every pass, called as
    pass(class_name, image_dataset, masks, preds, file_names, pred_masks).  what: the files' name in the error."""
    def after_class(class_name, image_dataset, masks, labels, preds, preds_image, file_names, details):
        if details is None or "masks" not in details:
            raise ValueError(f"{what} need the masks at the pixel F1-max threshold (f1_max=True, return_masks=True)")
        pred_masks = details["kept masks"] if defects is not None else details["masks"]
        for write in passes:
            write(class_name, image_dataset, masks, preds, file_names, pred_masks)
    return after_class


def overlay_callback(save_path: str, dataset: str, device, alpha: float, limit=None, thickness: int = 1, colormap: str = "jet",
                     batch_size: int = 32, loader_kwargs=None, defects=None, written=None):
    """-> the after_class callable that runs write_overlays for the class (mask_callback picks the predicted masks).
    written: None or a dict that receives {class name: paths}."""
    def overlays(class_name, image_dataset, masks, preds, file_names, pred_masks):
        folder = os.path.join(save_path, "overlays", dataset, class_name)
        paths = write_overlays(folder, image_dataset, masks, preds, file_names, pred_masks, device, alpha=alpha, limit=limit,
                               thickness=thickness, colormap=colormap, batch_size=batch_size, loader_kwargs=loader_kwargs)
        if written is not None:
            written[class_name] = paths
    return mask_callback("overlays", defects, overlays)


def check_files(one_process: str, needs_save_path: str, save_path, overlay, overlay_thickness, overlay_colormap) -> None:
    """what evaluate refuses before it writes overlays or masks; the two messages are the caller's"""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise ValueError(one_process)
    if save_path is None:
        raise ValueError(needs_save_path)
    if overlay is not None and (not 0.0 <= float(overlay) <= 1.0
                                or not 0 <= int(overlay_thickness) <= engine.OVERLAY_MAX_THICKNESS):
        raise ValueError("evaluate: overlay takes an alpha in 0 .. 1 and overlay_thickness 0 .. 8")
    engine.overlay_lut(overlay_colormap)


def own_masks_only(rows, details, return_masks: bool):
    """-> (rows, details) with return_masks; else rows, and the masks that were asked for on the files' behalf are dropped"""
    if return_masks:
        return rows, details
    for d in details.values():
        for key in ("masks", "kept masks", "support nearest"):
            d.pop(key, None)
    return rows


def evaluate(model, image_datasets, text_embeddings, device, img_size: int, dataset: str, batch_size: int = 32,
             loader_kwargs=None, logger=None, use_iqm: bool = True, device_metrics: bool = False, aupro_limit=None,
             f1_max: bool = False, return_masks: bool = False, defects=None, save_path=None, support=None,
             support_weight: float = SUPPORT_WEIGHT, support_form=None, support_datasets=None, coreset=None,
             coreset_dim: int = 128, tiles=None, tile_overlap: int = TILE_OVERLAP, overlay=None, overlay_limit=None,
             overlay_thickness: int = 1, overlay_colormap: str = "jet", overlay_written=None):
    """eval_tiled.evaluate; overlay: None, which is eval_tiled.evaluate and nothing else, or ALPHA in 0 .. 1: every class's
    overlays are written under <save_path>/overlays/<dataset>/<class>/ right after its row is computed (write_overlays;
    overlay_limit, overlay_thickness and overlay_colormap are its limit, thickness and colormap; overlay_written: None or
    a dict that receives {class name: paths}).  overlay implies f1_max and needs save_path; the rows and the return
    value are those of eval_tiled.evaluate with f1_max=True.  One process only."""
    where = (model, image_datasets, text_embeddings, device, img_size, dataset)
    below = dict(batch_size=batch_size, loader_kwargs=loader_kwargs, logger=logger, use_iqm=use_iqm,
                 device_metrics=device_metrics, aupro_limit=aupro_limit, f1_max=f1_max, return_masks=return_masks,
                 defects=defects, save_path=save_path, support=support, support_weight=support_weight,
                 support_form=support_form, support_datasets=support_datasets, coreset=coreset, coreset_dim=coreset_dim)
    if overlay is None:
        return ET.evaluate(*where, **below, tiles=tiles, tile_overlap=tile_overlap)
    check_files("overlays are written by one process (sharded evaluation with overlays is not part of it)",
                "evaluate: overlay needs save_path (the overlays go to <save_path>/overlays)", save_path, overlay,
                overlay_thickness, overlay_colormap)
    after = overlay_callback(save_path, dataset, device, float(overlay), limit=overlay_limit, thickness=int(overlay_thickness),
                             colormap=overlay_colormap, batch_size=ET.frames_per_batch(batch_size, tiles),
                             loader_kwargs=loader_kwargs, defects=defects, written=overlay_written)
    rows, details = ET.evaluate_details(*where, None if tiles is None else (tiles, tile_overlap),
                                        **dict(below, f1_max=True, return_masks=True), after_class=after)
    return own_masks_only(rows, details, return_masks)


def build_parser() -> argparse.ArgumentParser:
    parser = ET.build_parser()
    parser.add_argument("--overlay", type=float, nargs="?", const=OVERLAY_ALPHA, default=None, metavar="ALPHA",
                        help="write <save_path>/overlays/<dataset>/<class>/<name>.png: frame, heat map and ground truth "
                             "panels rendered on the GPU; ALPHA (0.5 when given without a value) is the frame's weight in "
                             "the blends; implies --f1max")
    parser.add_argument("--overlay_limit", type=int, default=None, metavar="N",
                        help="only the first N images of each class, in file order (default: all)")
    parser.add_argument("--overlay_thickness", type=int, default=1, metavar="T",
                        help="reach of the mask contours in pixels, 0 .. 8 (0 draws none)")
    parser.add_argument("--overlay_colormap", choices=list(engine.OVERLAY_LUTS), default="jet")
    return parser


def _check_arguments(parser: argparse.ArgumentParser, args) -> None:
    """this script's checks (the alpha where --overlay is given: eval_png.py writes masks without it), then eval_tiled's"""
    if args.overlay is not None and not 0.0 <= args.overlay <= 1.0:
        parser.error("--overlay takes the frame's weight in 0 .. 1")
    if args.overlay_limit is not None and args.overlay_limit < 0:
        parser.error("--overlay_limit takes a number of images")
    if not 0 <= args.overlay_thickness <= engine.OVERLAY_MAX_THICKNESS:
        parser.error("--overlay_thickness takes 0 .. 8 pixels")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        parser.error("--overlay runs in one process: sharded evaluation with overlays is not part of this script")
    ET._check_arguments(parser, args)


def open_session(args, name: str):
    """eval_last.open_session with the datasets at the canvas size of --tiles: -> (session, where), where = the six
    leading arguments of evaluate"""
    canvas = args.img_size if args.tiles is None else ET.tile_geometry(args.img_size, args.tiles, args.tile_overlap)[3]
    session = EL.open_session(args, name, canvas)
    return session, (session.model, session.image_datasets, session.text_embeddings, session.device, args.img_size,
                     args.dataset)


def overlay_keywords(args) -> dict:
    """the keywords of evaluate that --tiles and the --overlay flags set"""
    return dict(tiles=args.tiles, tile_overlap=args.tile_overlap, overlay=args.overlay, overlay_limit=args.overlay_limit,
                overlay_thickness=args.overlay_thickness, overlay_colormap=args.overlay_colormap)


def run(parser: argparse.ArgumentParser, argv=None):
    """Without --overlay: eval_tiled.run.  With it: the session (the datasets built at the canvas size with --tiles, at
    --img_size without) and this module's evaluate."""
    args = parser.parse_args(argv)
    if args.overlay is None:
        return ET.run(parser, argv)
    _check_arguments(parser, args)
    session, where = open_session(args, __name__)
    written = {}
    rows, details = evaluate(*where, f1_max=True, return_masks=True, **ET.session_keywords(args, session),
                             **overlay_keywords(args), overlay_written=written)
    for name, d in details.items():
        session.logger.info("%s: pixel threshold %.9g, image threshold %s (normalised units); %d overlays", name,
                            d["pixel threshold"], d["image threshold"], len(written.get(name, ())))
    ED.log_table(session.logger, rows)
    return rows


def main(argv=None):
    return run(build_parser(), argv)


if __name__ == "__main__":
    main()
