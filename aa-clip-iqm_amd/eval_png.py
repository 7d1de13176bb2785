"""eval_overlay.py with the PNG encoder on the GPU: its arguments and steps, plus

  --overlay_encoder device|pillow   who compresses the overlays of --overlay.  pillow (default) is eval_overlay.py's pass:
                             the panels come to the host and at most 8 threads encode them with Pillow.  device: every
                             batch of panels goes through engine.png_encode (csrc/png.hip: row filters and a segmented
                             deflate, two launches per batch), the offsets are read once, the used part of the payload
                             comes to the host in one copy, and the threads only wrap each stream into a file (signature,
                             IHDR, IDAT, IEND and their CRC-32) and write it.  The files of the two encoders decode to the
                             same pixels; their BYTES differ (another choice of filters, distance-1 matches only).
  --masks_png                also write <save_path>/masks/<dataset>/<class>/<name>.png: the predicted mask at the class's
                             pixel F1-max threshold (with --defects the mask that the area filter kept) as a one-channel
                             PNG of 0 / 255, named like the overlays, encoded on the device with --overlay_encoder device
                             and by Pillow otherwise.  Implies --f1max; works without --overlay.

The definition of every byte of the device encoder is forward_utils.png_encode_host.  Under WORLD_SIZE > 1 both flags are
refused, like --overlay.  Without either flag the script prints and writes exactly what eval_overlay.py does.
evaluate(..., overlay_encoder=..., masks_png=...) is the function form; write_overlays and write_masks are the passes
over one class.

python eval_png.py --save_path ... [--overlay [ALPHA]] [--overlay_encoder device] [--masks_png] [every argument of eval_overlay.py]
"""
from __future__ import annotations

import argparse
import concurrent.futures
import os

import numpy as np
import torch

import eval_defects as ED
import eval_overlay as EO
import eval_tiled as ET
from aaclip_hip import engine
from forward_utils import SUPPORT_WEIGHT, TILE_OVERLAP, png_file

ENCODERS = ("device", "pillow")


def _write_png(path: str, payload: np.ndarray, lo: int, hi: int, H: int, W: int, C: int) -> None:
    with open(path, "wb") as f:
        f.write(png_file(payload[lo:hi], H, W, C))


def _save_mask(path: str, mask: np.ndarray) -> None:
    from PIL import Image
    Image.fromarray(mask, "L").save(path, format="PNG")


def submit_device_pngs(pool, pixels: torch.Tensor, paths) -> list:
    """pixels uint8 [b, H, W, C] or [b, H, W] on the device -> the futures of its b files: one engine.png_encode, the
    offsets read once, the used part of the payload brought to the host in one copy; the pool's threads wrap the streams
    into files and write them."""
    payload, offsets = engine.png_encode(pixels)
    offsets = offsets.cpu().tolist()
    host = payload[:offsets[-1]].cpu().numpy()
    H, W = int(pixels.shape[1]), int(pixels.shape[2])
    C = int(pixels.shape[3]) if pixels.dim() == 4 else 1
    return [pool.submit(_write_png, path, host, offsets[i], offsets[i + 1], H, W, C) for i, path in enumerate(paths)]


def write_overlays(folder: str, image_dataset, masks, preds, file_names, pred_masks, device, alpha: float = EO.OVERLAY_ALPHA,
                   limit=None, thickness: int = 1, colormap: str = "jet", batch_size: int = 32, loader_kwargs=None,
                   encoder: str = "pillow") -> list:
    """eval_overlay.write_overlays, which it is for encoder="pillow"; with encoder="device" the same pass with every batch
    of panels compressed on the GPU (submit_device_pngs).  The files decode to the same pixels.  -> the paths written."""
    if encoder not in ENCODERS:
        raise ValueError(f"overlays: encoder must be one of {ENCODERS}, got {encoder!r}")
    submit = submit_device_pngs if encoder == "device" else EO._submit_pillow
    return EO._overlay_pass(submit, folder, image_dataset, masks, preds, file_names, pred_masks, device, alpha, limit,
                            thickness, colormap, batch_size, loader_kwargs)


def write_masks(folder: str, file_names, pred_masks, device, encoder: str = "pillow", batch_size: int = 32) -> list:
    """pred_masks [N, H, W], non-zero = set (a device tensor or a host array) -> one one-channel PNG of 0 / 255 per image
    under `folder`, named by eval_overlay.overlay_paths (two images with one name are a ValueError before anything is
    written).  encoder "device": engine.png_encode per batch; "pillow": Pillow on at most 8 threads.  -> the paths."""
    if encoder not in ENCODERS:
        raise ValueError(f"masks: encoder must be one of {ENCODERS}, got {encoder!r}")
    if len(pred_masks) != len(file_names):
        raise ValueError(f"masks: {len(pred_masks)} masks and {len(file_names)} file names")
    paths = EO.overlay_paths(folder, list(file_names))
    if not paths:
        return paths
    os.makedirs(folder, exist_ok=True)
    H, W = (int(v) for v in pred_masks.shape[-2:])
    pending = []
    with concurrent.futures.ThreadPoolExecutor(max_workers=EO.OVERLAY_WRITERS) as pool:
        for lo in range(0, len(paths), batch_size):
            rows = slice(lo, min(lo + batch_size, len(paths)))
            part = pred_masks[rows]
            if encoder == "device":
                part = (part if torch.is_tensor(part) else torch.from_numpy(np.ascontiguousarray(part))).to(device)
                pixels = ((part.reshape(-1, H, W) != 0).to(torch.uint8) * 255).contiguous()
                futures = submit_device_pngs(pool, pixels, paths[rows])
            else:
                part = part.cpu().numpy() if torch.is_tensor(part) else np.asarray(part)
                pixels = ((part.reshape(-1, H, W) != 0) * 255).astype(np.uint8)
                futures = [pool.submit(_save_mask, path, pixels[i]) for i, path in enumerate(paths[rows])]
            for f in pending:
                f.result()
            pending = futures
        for f in pending:
            f.result()
    return paths


def png_callback(save_path: str, dataset: str, device, overlay=None, encoder: str = "pillow", masks_png: bool = False,
                 limit=None, thickness: int = 1, colormap: str = "jet", batch_size: int = 32, loader_kwargs=None,
                 defects=None, written=None, masks_written=None):
    """-> the after_class callable that writes a class's overlays (overlay: None or ALPHA) and its masks (masks_png) from
    the predicted masks that eval_overlay.mask_callback picks.  written / masks_written: None or dicts that receive
    {class name: paths}."""
    def overlays(class_name, image_dataset, masks, preds, file_names, pred_masks):
        paths = write_overlays(os.path.join(save_path, "overlays", dataset, class_name), image_dataset, masks, preds,
                               file_names, pred_masks, device, alpha=overlay, limit=limit, thickness=thickness,
                               colormap=colormap, batch_size=batch_size, loader_kwargs=loader_kwargs, encoder=encoder)
        if written is not None:
            written[class_name] = paths

    def mask_files(class_name, image_dataset, masks, preds, file_names, pred_masks):
        paths = write_masks(os.path.join(save_path, "masks", dataset, class_name), file_names, pred_masks, device,
                            encoder=encoder, batch_size=batch_size)
        if masks_written is not None:
            masks_written[class_name] = paths

    passes = ([overlays] if overlay is not None else []) + ([mask_files] if masks_png else [])
    return EO.mask_callback("overlays and masks", defects, *passes)


def check_encoder(overlay_encoder) -> None:
    if overlay_encoder not in ENCODERS:
        raise ValueError(f"evaluate: overlay_encoder must be one of {ENCODERS}, got {overlay_encoder!r}")


def files_callback(save_path, dataset: str, device, batch_size: int, loader_kwargs, defects, tiles, *, overlay, overlay_limit,
                   overlay_thickness, overlay_colormap, overlay_written, overlay_encoder, masks_png, masks_written):
    """evaluate's keywords -> what it refuses before it writes files (eval_overlay.check_files), then its png_callback"""
    EO.check_files("overlays and masks are written by one process (sharded evaluation with them is not part of it)",
                   "evaluate: overlay and masks_png need save_path (the files go to <save_path>/overlays and /masks)",
                   save_path, overlay, overlay_thickness, overlay_colormap)
    return png_callback(save_path, dataset, device, overlay=None if overlay is None else float(overlay),
                        encoder=overlay_encoder, masks_png=masks_png, limit=overlay_limit, thickness=int(overlay_thickness),
                        colormap=overlay_colormap, batch_size=ET.frames_per_batch(batch_size, tiles),
                        loader_kwargs=loader_kwargs, defects=defects, written=overlay_written, masks_written=masks_written)


def evaluate(model, image_datasets, text_embeddings, device, img_size: int, dataset: str, batch_size: int = 32,
             loader_kwargs=None, logger=None, use_iqm: bool = True, device_metrics: bool = False, aupro_limit=None,
             f1_max: bool = False, return_masks: bool = False, defects=None, save_path=None, support=None,
             support_weight: float = SUPPORT_WEIGHT, support_form=None, support_datasets=None, coreset=None,
             coreset_dim: int = 128, tiles=None, tile_overlap: int = TILE_OVERLAP, overlay=None, overlay_limit=None,
             overlay_thickness: int = 1, overlay_colormap: str = "jet", overlay_written=None, overlay_encoder: str = "pillow",
             masks_png: bool = False, masks_written=None):
    """eval_overlay.evaluate, which it is for overlay_encoder="pillow" without masks_png.  overlay_encoder "device"
    compresses the overlays on the GPU; masks_png also writes every class's predicted masks under
    <save_path>/masks/<dataset>/<class>/ (masks_written: None or a dict that receives {class name: paths}), with or without
    overlay.  Either implies f1_max and needs save_path; the rows and the return value are those of eval_overlay.evaluate
    with f1_max=True.  One process only."""
    where = (model, image_datasets, text_embeddings, device, img_size, dataset)
    below = dict(batch_size=batch_size, loader_kwargs=loader_kwargs, logger=logger, use_iqm=use_iqm,
                 device_metrics=device_metrics, aupro_limit=aupro_limit, f1_max=f1_max, return_masks=return_masks,
                 defects=defects, save_path=save_path, support=support, support_weight=support_weight,
                 support_form=support_form, support_datasets=support_datasets, coreset=coreset, coreset_dim=coreset_dim)
    check_encoder(overlay_encoder)
    if not masks_png and (overlay is None or overlay_encoder == "pillow"):
        return EO.evaluate(*where, **below, tiles=tiles, tile_overlap=tile_overlap, overlay=overlay,
                           overlay_limit=overlay_limit, overlay_thickness=overlay_thickness,
                           overlay_colormap=overlay_colormap, overlay_written=overlay_written)
    after = files_callback(save_path, dataset, device, batch_size, loader_kwargs, defects, tiles, overlay=overlay,
                           overlay_limit=overlay_limit, overlay_thickness=overlay_thickness,
                           overlay_colormap=overlay_colormap, overlay_written=overlay_written,
                           overlay_encoder=overlay_encoder, masks_png=masks_png, masks_written=masks_written)
    rows, details = ET.evaluate_details(*where, None if tiles is None else (tiles, tile_overlap),
                                        **dict(below, f1_max=True, return_masks=True), after_class=after)
    return EO.own_masks_only(rows, details, return_masks)


def build_parser() -> argparse.ArgumentParser:
    parser = EO.build_parser()
    parser.add_argument("--overlay_encoder", choices=list(ENCODERS), default="pillow",
                        help="who compresses the PNGs: the GPU (engine.png_encode; the threads only wrap and write) or "
                             "Pillow on the host; the files decode to the same pixels, their bytes differ")
    parser.add_argument("--masks_png", action="store_true",
                        help="write <save_path>/masks/<dataset>/<class>/<name>.png: the predicted mask at the pixel F1-max "
                             "threshold (with --defects the kept mask) as a one-channel PNG of 0 / 255; implies --f1max")
    return parser


def run(parser: argparse.ArgumentParser, argv=None):
    """Without --masks_png and without --overlay with --overlay_encoder device: eval_overlay.run.  Else its checks and
    session and this module's evaluate."""
    args = parser.parse_args(argv)
    if not args.masks_png and (args.overlay is None or args.overlay_encoder == "pillow"):
        return EO.run(parser, argv)
    EO._check_arguments(parser, args)
    session, where = EO.open_session(args, __name__)
    written, masks_written = {}, {}
    rows, details = evaluate(*where, f1_max=True, return_masks=True, **ET.session_keywords(args, session),
                             **EO.overlay_keywords(args), overlay_written=written, overlay_encoder=args.overlay_encoder,
                             masks_png=args.masks_png, masks_written=masks_written)
    for name, d in details.items():
        session.logger.info("%s: pixel threshold %.9g, image threshold %s (normalised units); %d overlays, %d masks (%s)",
                            name, d["pixel threshold"], d["image threshold"], len(written.get(name, ())),
                            len(masks_written.get(name, ())), args.overlay_encoder)
    ED.log_table(session.logger, rows)
    return rows


def main(argv=None):
    return run(build_parser(), argv)


if __name__ == "__main__":
    main()
