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
import logging
import os

import numpy as np
import torch

import eval_defects as ED
import eval_last as EL
import eval_overlay as EO
import eval_tiled as ET
import test_last as TL
from aaclip_hip import engine
from forward_utils import SUPPORT_WEIGHT, TILE_OVERLAP, png_file, render_overlays

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
    if encoder == "pillow":
        return EO.write_overlays(folder, image_dataset, masks, preds, file_names, pred_masks, device, alpha=alpha, limit=limit,
                                 thickness=thickness, colormap=colormap, batch_size=batch_size, loader_kwargs=loader_kwargs)
    n = len(file_names) if limit is None else max(0, min(int(limit), len(file_names)))
    if len(image_dataset) != len(file_names) or len(preds) != len(file_names):
        raise ValueError(f"overlays: {len(image_dataset)} images, {len(preds)} maps and {len(file_names)} file names")
    paths = EO.overlay_paths(folder, list(file_names)[:n])       # before anything is written
    if n == 0:
        return paths
    H, W = (int(v) for v in preds.shape[-2:])
    record = EO._range_record(preds, device)
    to_device = lambda a, dtype: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(device).to(dtype)
    os.makedirs(folder, exist_ok=True)
    loader = torch.utils.data.DataLoader(image_dataset, batch_size=batch_size, shuffle=False, **(loader_kwargs or {}))
    done, pending = 0, []
    with concurrent.futures.ThreadPoolExecutor(max_workers=EO.OVERLAY_WRITERS) as pool:
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
            pending = submit_device_pngs(pool, panels, paths[done:done + b])
            done += b
        for f in pending:
            f.result()
    if done != n:
        raise ValueError(f"overlays: the dataset gave {done} of {n} images")
    return paths


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
    """-> the after_class callable that writes a class's overlays (overlay: None or ALPHA) and its masks (masks_png); the
    predicted masks are details["kept masks"] with defects, else details["masks"].  written / masks_written: None or
    dicts that receive {class name: paths}."""
    def after_class(class_name, image_dataset, masks, labels, preds, preds_image, file_names, details):
        if details is None or "masks" not in details:
            raise ValueError("overlays and masks need the masks at the pixel F1-max threshold (f1_max=True, return_masks=True)")
        pred_masks = details["kept masks"] if defects is not None else details["masks"]
        if overlay is not None:
            paths = write_overlays(os.path.join(save_path, "overlays", dataset, class_name), image_dataset, masks, preds,
                                   file_names, pred_masks, device, alpha=overlay, limit=limit, thickness=thickness,
                                   colormap=colormap, batch_size=batch_size, loader_kwargs=loader_kwargs, encoder=encoder)
            if written is not None:
                written[class_name] = paths
        if masks_png:
            paths = write_masks(os.path.join(save_path, "masks", dataset, class_name), file_names, pred_masks, device,
                                encoder=encoder, batch_size=batch_size)
            if masks_written is not None:
                masks_written[class_name] = paths
    return after_class


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
    if overlay_encoder not in ENCODERS:
        raise ValueError(f"evaluate: overlay_encoder must be one of {ENCODERS}, got {overlay_encoder!r}")
    if not masks_png and (overlay is None or overlay_encoder == "pillow"):
        return EO.evaluate(*where, batch_size=batch_size, loader_kwargs=loader_kwargs, logger=logger, use_iqm=use_iqm,
                           device_metrics=device_metrics, aupro_limit=aupro_limit, f1_max=f1_max, return_masks=return_masks,
                           defects=defects, save_path=save_path, support=support, support_weight=support_weight,
                           support_form=support_form, support_datasets=support_datasets, coreset=coreset,
                           coreset_dim=coreset_dim, tiles=tiles, tile_overlap=tile_overlap, overlay=overlay,
                           overlay_limit=overlay_limit, overlay_thickness=overlay_thickness,
                           overlay_colormap=overlay_colormap, overlay_written=overlay_written)
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise ValueError("overlays and masks are written by one process (sharded evaluation with them is not part of it)")
    if save_path is None:
        raise ValueError("evaluate: overlay and masks_png need save_path (the files go to <save_path>/overlays and /masks)")
    if overlay is not None and (not 0.0 <= float(overlay) <= 1.0
                                or not 0 <= int(overlay_thickness) <= engine.OVERLAY_MAX_THICKNESS):
        raise ValueError("evaluate: overlay takes an alpha in 0 .. 1 and overlay_thickness 0 .. 8")
    engine.overlay_lut(overlay_colormap)
    if coreset is not None and support is None:
        raise ValueError("evaluate: coreset needs support=K")
    after = png_callback(save_path, dataset, device, overlay=None if overlay is None else float(overlay),
                         encoder=overlay_encoder, masks_png=masks_png, limit=overlay_limit, thickness=int(overlay_thickness),
                         colormap=overlay_colormap, batch_size=batch_size if tiles is None else
                         max(1, batch_size // (int(tiles) ** 2)), loader_kwargs=loader_kwargs, defects=defects,
                         written=overlay_written, masks_written=masks_written)
    if tiles is not None:
        rows, details = ET.evaluate_details(*where, (tiles, tile_overlap), batch_size=batch_size, loader_kwargs=loader_kwargs,
                                            logger=logger, use_iqm=use_iqm, device_metrics=device_metrics,
                                            aupro_limit=aupro_limit, f1_max=True, return_masks=True, defects=defects,
                                            save_path=save_path, support=support, support_weight=support_weight,
                                            support_form=support_form, support_datasets=support_datasets, coreset=coreset,
                                            coreset_dim=coreset_dim, after_class=after)
    else:
        banks = None
        if support is not None:
            core = {} if coreset is None else {"coreset": coreset, "coreset_dim": coreset_dim}
            banks, image_datasets = EL.support_banks(model, image_datasets, support, device, img_size, form=support_form,
                                                     support_datasets=support_datasets, batch_size=batch_size, **core)
            if logger and coreset is not None:
                EL.log_coreset(logger, banks)
        details = {}
        extra = {} if defects is None else {"defects": defects}
        if banks is not None:
            extra.update(support=banks, support_weight=support_weight)
        rows = EL.evaluate_rows(model, image_datasets, text_embeddings, device, img_size, dataset, batch_size=batch_size,
                                loader_kwargs=loader_kwargs, logger=logger, use_iqm=use_iqm, device_metrics=device_metrics,
                                fpr_limit=aupro_limit, f1_max=True, details=details, return_masks=True, after_class=after,
                                **extra)
        if defects is not None:
            ED.write_defects(save_path, dataset, details)
    if return_masks:
        return rows, details
    for d in details.values():               # the masks were asked for on the files' behalf only
        for key in ("masks", "kept masks", "support nearest"):
            d.pop(key, None)
    return rows


def build_parser() -> argparse.ArgumentParser:
    parser = EO.build_parser()
    parser.add_argument("--overlay_encoder", choices=list(ENCODERS), default="pillow",
                        help="who compresses the PNGs: the GPU (engine.png_encode; the threads only wrap and write) or "
                             "Pillow on the host; the files decode to the same pixels, their bytes differ")
    parser.add_argument("--masks_png", action="store_true",
                        help="write <save_path>/masks/<dataset>/<class>/<name>.png: the predicted mask at the pixel F1-max "
                             "threshold (with --defects the kept mask) as a one-channel PNG of 0 / 255; implies --f1max")
    return parser


def _check_arguments(parser: argparse.ArgumentParser, args) -> None:
    """eval_overlay's checks; without --overlay they run against its default alpha, which passes"""
    probe = args if args.overlay is not None else argparse.Namespace(**dict(vars(args), overlay=EO.OVERLAY_ALPHA))
    EO._check_arguments(parser, probe)


def run(parser: argparse.ArgumentParser, argv=None):
    """Without --masks_png and without --overlay with --overlay_encoder device: eval_overlay.run.  Else its steps and this
    module's evaluate."""
    args = parser.parse_args(argv)
    if not args.masks_png and (args.overlay is None or args.overlay_encoder == "pillow"):
        return EO.run(parser, argv)
    _check_arguments(parser, args)
    from dataset import DATA_PATH, BaseSingleClassDataset, get_dataset
    from forward_utils import get_adapted_text_embedding
    from model.adapter import AdaptedCLIP
    from model.clip import create_model
    S = args.img_size
    C = S if args.tiles is None else ET.tile_geometry(S, args.tiles, args.tile_overlap)[3]
    TL.setup_seed(args.seed)
    os.makedirs(args.save_path, exist_ok=True)
    logger = logging.getLogger(__name__)
    logging.basicConfig(filename=os.path.join(args.save_path, "test.log"), encoding="utf-8", level=logging.INFO)
    logger.info("args: %s", vars(args))
    if not torch.cuda.is_available():
        raise RuntimeError("the AA-CLIP HIP path needs an MI355X; there is no CPU fallback")
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1))
    torch.cuda.set_device(device)
    clip_model = create_model(model_name=args.model_name, img_size=S, device=device, pretrained="openai",
                              require_pretrained=True, precision=args.precision)
    clip_model.eval()
    model = AdaptedCLIP(clip_model=clip_model, text_adapt_weight=args.text_adapt_weight,
                        image_adapt_weight=args.image_adapt_weight, text_adapt_until=args.text_adapt_until,
                        image_adapt_until=args.image_adapt_until, relu=args.relu,
                        iqm_hidden_size=args.iqm_hidden_size, iqm_num_layers=args.iqm_num_layers,
                        iqm_num_heads=args.iqm_num_heads).to(device)
    model.eval()
    adapt_text = EL.load_adapters(model, args.save_path, logger)
    image_datasets = get_dataset(args.dataset, C, None, args.shot, "test", logger=logger,
                                 device_preprocess=args.device_preprocess)
    with torch.no_grad():
        text_embeddings = get_adapted_text_embedding(model if adapt_text else clip_model, args.dataset, device)
    support_sets = None
    if args.support is not None and args.support_meta:
        support_sets = {c: BaseSingleClassDataset(DATA_PATH[args.dataset], args.support_meta, C, c,
                                                  device_preprocess=args.device_preprocess) for c in image_datasets}
    written, masks_written = {}, {}
    rows, details = evaluate(model, image_datasets, text_embeddings, device, S, args.dataset, batch_size=args.image_batch_size,
                             loader_kwargs={"num_workers": 4, "pin_memory": True}, logger=logger, use_iqm=args.iqm == "on",
                             device_metrics=args.device_metrics, aupro_limit=args.aupro, f1_max=True, return_masks=True,
                             defects=args.defects, save_path=args.save_path, support=args.support,
                             support_weight=args.support_weight, support_form=args.support_form,
                             support_datasets=support_sets, coreset=args.support_coreset,
                             coreset_dim=args.support_coreset_dim, tiles=args.tiles, tile_overlap=args.tile_overlap,
                             overlay=args.overlay, overlay_limit=args.overlay_limit, overlay_thickness=args.overlay_thickness,
                             overlay_colormap=args.overlay_colormap, overlay_written=written,
                             overlay_encoder=args.overlay_encoder, masks_png=args.masks_png, masks_written=masks_written)
    for name, d in details.items():
        logger.info("%s: pixel threshold %.9g, image threshold %s (normalised units); %d overlays, %d masks (%s)", name,
                    d["pixel threshold"], d["image threshold"], len(written.get(name, ())),
                    len(masks_written.get(name, ())), args.overlay_encoder)
    table = ED.format_table(rows)
    logger.info("final results:\n%s", table)
    print(table)
    return rows


def main(argv=None):
    return run(build_parser(), argv)


if __name__ == "__main__":
    main()
