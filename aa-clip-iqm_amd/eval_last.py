"""The evaluation harness of test_last.py with the metrics on the GPU and with the IQM branch this project's own
training saves.  test_last.py itself stays the reference-shaped script with the host metrics; this module adds, with
the same names and arguments:

  get_predictions(..., on_device=False)   True: masks (uint8 0 / 1), maps and image scores stay tensors on the device,
                                          no per-batch copy to the host
  evaluate(..., device_metrics=False)     True: one class's tensors live on the GPU at a time and
                                          forward_utils.metrics_eval_device computes the row there (a radix sort and
                                          exact curve sums: the numbers sklearn gives), instead of copying every batch
                                          to the host for sklearn; the rows are the very rows of test_last.evaluate
  load_adapters(model, save_path, logger) as test_last.load_adapters, and -- unless a separate iqm_branch.pth exists,
                                          which keeps precedence -- the IQM branch from the "iqm_branch" entry that
                                          train.train_image_adapter writes into image_adapter_<epoch>.pth; test_last.py
                                          evaluates the branch with its seeded initialisation after training
  evaluate_rows(..., device_metrics=False, fpr_limit=None)
                                          the loop behind evaluate(device_metrics=True), for either metrics path; a
                                          number as fpr_limit adds the column "pixel AUPRO": the per-region overlap curve
                                          integrated up to that false-positive rate (forward_utils.pro_eval on the host,
                                          pro_eval_device on the GPU).  eval_aupro.py is the script with the --aupro flag;
                                          this script's arguments and evaluate() stay test_last's plus --device_metrics
                                          f1_max=True adds "pixel F1-max" and "image F1-max", the best F1 over every
                                          threshold (forward_utils.f1max_eval / engine.f1max_metrics); eval_metrics.py is
                                          the script with the --f1max flag
                                          defects=MIN_AREA (with f1_max) adds the region-level columns of the defect
                                          instances at the pixel F1-max threshold (forward_utils.defects_eval /
                                          engine.defects_at_threshold); eval_defects.py is the script with --defects
                                          support={class: engine.SupportBank} adds the few-shot memory-bank term to the
                                          text-anchor map before the IQM fusion (forward_utils.support_anomaly_map;
                                          support_banks builds the banks); eval_support.py is the script with --support
                                          (support_banks(coreset=R) reduces every bank to the greedy coreset of the
                                          share R of its rows, an engine.CoresetBank; eval_coreset.py is the script
                                          with --support_coreset)
  open_session(args, name, canvas)        the set-up of every script of the tower, once: seed, test.log, device, model,
                                          adapters, datasets, text embeddings, --support_meta datasets
  main(argv)                              the arguments and steps of test_last.main plus --device_metrics

python eval_last.py --save_path ... [--device_metrics] [every argument of test_last.py]
"""
from __future__ import annotations

import argparse
import collections
import logging
import os
from glob import glob
from typing import Dict, List

import numpy as np
import torch

import test_last as TL
from aaclip_hip import engine
from aaclip_hip.shard import gather_predictions, shard_range
from dataset import DOMAINS
from forward_utils import (DEFECT_COLS, IMAGE_F1_COL, PIXEL_F1_COL, SUPPORT_WEIGHT, calculate_anomaly_map, image_score,
                           metrics_eval, metrics_eval_device, support_anomaly_map)

AUPRO_COL = "pixel AUPRO"
F1_COLS = [PIXEL_F1_COL, IMAGE_F1_COL]


def get_predictions(model, class_text_embeddings: torch.Tensor, test_loader, device, img_size: int,
                    dataset: str = "MVTec", use_iqm: bool = True, on_device: bool = False):
    """test_last.get_predictions; on_device: masks [N,1,S,S] uint8, preds [N,S,S] and preds_image [N] fp32 are device
    tensors (labels [N] and the file names stay on the host)."""
    if not on_device:
        return TL.get_predictions(model, class_text_embeddings, test_loader, device, img_size, dataset, use_iqm)
    masks, labels, preds, preds_image, file_names = [], [], [], [], []
    domain = DOMAINS[dataset]
    for input_data in test_loader:
        image = input_data["image"].to(device, non_blocking=True)
        assert len(set(input_data["class_name"])) == 1, "mixed class not supported"
        masks.append((input_data["mask"].to(device, non_blocking=True) != 0).to(torch.uint8))
        labels.append(np.asarray(torch.as_tensor(input_data["label"]).cpu().numpy()))
        file_names.extend(input_data["file_name"])
        if image.dtype == torch.uint8:                       # raw HWC frames: resize + normalise on the GPU
            image = engine.preprocess(image, img_size)
        epoch_text_feature = class_text_embeddings.unsqueeze(0).repeat(image.size(0), 1, 1) if use_iqm else None
        patch_features, det_feature, iqm_outputs = model(image, text_embeddings=epoch_text_feature)
        preds_image.append(image_score(det_feature, class_text_embeddings).float())
        final_map = calculate_anomaly_map(patch_features, class_text_embeddings, img_size, domain=domain)
        if iqm_outputs is not None:
            final_map = engine.iqm_map(patch_features, iqm_outputs.last_hidden_state, img_size, base=final_map,
                                       w_base=TL.TEXT_WEIGHT, w_iqm=TL.IQM_WEIGHT)
        preds.append(final_map)
    return (torch.cat(masks, dim=0), np.concatenate(labels, axis=0), torch.cat(preds, dim=0),
            torch.cat(preds_image, dim=0), file_names)


def get_predictions_support(model, class_text_embeddings: torch.Tensor, test_loader, device, img_size: int,
                            dataset: str = "MVTec", use_iqm: bool = True, on_device: bool = False, support=None,
                            support_weight: float = SUPPORT_WEIGHT, nearest: list = None):
    """get_predictions with the class's few-shot bank (its signature is test_last's plus on_device and stays so; this is
    the function with the further keywords).  support: an engine.SupportBank, or None, which is get_predictions itself.
    With a bank the text-anchor map becomes calculate_anomaly_map(...) + support_weight * (the nearest-patch distance to
    the bank, blurred, upsampled and summed over the levels like the text map: forward_utils.support_anomaly_map) BEFORE
    the IQM fusion, which is unchanged.  nearest: a list that then receives, per batch, the per-level int32 [b, P]
    indices of the nearest bank rows.  on_device as in get_predictions."""
    if support is None:
        return get_predictions(model, class_text_embeddings, test_loader, device, img_size, dataset, use_iqm, on_device)
    masks, labels, preds, preds_image, file_names = [], [], [], [], []
    domain = DOMAINS[dataset]
    for input_data in test_loader:
        image = input_data["image"].to(device, non_blocking=True)
        assert len(set(input_data["class_name"])) == 1, "mixed class not supported"
        if on_device:
            masks.append((input_data["mask"].to(device, non_blocking=True) != 0).to(torch.uint8))
        else:
            masks.append(np.asarray(input_data["mask"].cpu().numpy()))
        labels.append(np.asarray(torch.as_tensor(input_data["label"]).cpu().numpy()))
        file_names.extend(input_data["file_name"])
        if image.dtype == torch.uint8:
            image = engine.preprocess(image, img_size)
        epoch_text_feature = class_text_embeddings.unsqueeze(0).repeat(image.size(0), 1, 1) if use_iqm else None
        patch_features, det_feature, iqm_outputs = model(image, text_embeddings=epoch_text_feature)
        score = image_score(det_feature, class_text_embeddings)
        final_map = calculate_anomaly_map(patch_features, class_text_embeddings, img_size, domain=domain)
        batch_nearest = [] if nearest is not None else None
        final_map = support_anomaly_map(patch_features, support, img_size, domain=domain, base=final_map,
                                        weight=support_weight, nearest=batch_nearest)
        if nearest is not None:
            nearest.append(batch_nearest)
        if iqm_outputs is not None:
            final_map = engine.iqm_map(patch_features, iqm_outputs.last_hidden_state, img_size, base=final_map,
                                       w_base=TL.TEXT_WEIGHT, w_iqm=TL.IQM_WEIGHT)
        preds_image.append(score.float() if on_device else score.cpu().numpy())
        preds.append(final_map if on_device else final_map.cpu().numpy())
    cat = (lambda v: torch.cat(v, dim=0)) if on_device else (lambda v: np.concatenate(v, axis=0))
    return cat(masks), np.concatenate(labels, axis=0), cat(preds), cat(preds_image), file_names


def evaluate(model, image_datasets: Dict[str, torch.utils.data.Dataset], text_embeddings: Dict[str, torch.Tensor],
             device, img_size: int, dataset: str, batch_size: int = 32, loader_kwargs=None, logger=None,
             use_iqm: bool = True, device_metrics: bool = False) -> List[dict]:
    """test_last.evaluate; device_metrics: evaluate_rows with the metrics on the GPU"""
    if not device_metrics:
        return TL.evaluate(model, image_datasets, text_embeddings, device, img_size, dataset, batch_size=batch_size,
                           loader_kwargs=loader_kwargs, logger=logger, use_iqm=use_iqm)
    return evaluate_rows(model, image_datasets, text_embeddings, device, img_size, dataset, batch_size=batch_size,
                         loader_kwargs=loader_kwargs, logger=logger, use_iqm=use_iqm, device_metrics=True)


def evaluate_rows(model, image_datasets: Dict[str, torch.utils.data.Dataset], text_embeddings: Dict[str, torch.Tensor],
                  device, img_size: int, dataset: str, batch_size: int = 32, loader_kwargs=None, logger=None,
                  use_iqm: bool = True, device_metrics: bool = False, fpr_limit=None, f1_max: bool = False,
                  details: Dict[str, dict] = None, return_masks: bool = False, defects=None, support=None,
                  support_weight: float = SUPPORT_WEIGHT, bootstrap=None, after_class=None) -> List[dict]:
    """The per-class loop of test_last.evaluate for either metrics path.  device_metrics: the class's masks, maps and
    image scores stay on the GPU, the row comes from metrics_eval_device, and the tensors are released before the next
    class.  Under torch.distributed the shards are gathered as host arrays exactly as in test_last.evaluate (so the
    gloo rehearsal path keeps working) and the gathered arrays of a class are uploaded once.  fpr_limit: a
    false-positive rate in (0, 1] adds "pixel AUPRO" to every row and to the average; None leaves the rows as they are.
    f1_max: adds "pixel F1-max" and "image F1-max" likewise (forward_utils.f1max_eval; on the GPU from the sort that
    serves AUROC / AP).  details: with f1_max, a dict that receives, per class name, what metrics_eval's `details`
    receives: the thresholds of the operating points and, with return_masks=True, the class's predicted uint8 masks;
    beside them the class's "file_names", "labels" and raw "image scores" in the order of the maps.
    defects: None, or a min_area (needs f1_max): metrics_eval's keyword -- the three region-level columns of
    forward_utils.DEFECT_COLS in every row and in the average, the per-image lists of defects under details[class].
    support: None, or {class name: engine.SupportBank} (forward_utils.build_support_bank of the class's k normal images;
    under torch.distributed every rank builds the same bank itself): get_predictions_support's keyword for every class, weighted
    by support_weight.  With details and return_masks=True, details[class]["support nearest"] is then a list per tap
    level of int32 arrays [N, P, 2]: (shot, patch) = divmod(index of the nearest bank row, P) for every patch of every
    evaluated image -- which good patch it was compared with.  support=None changes nothing.
    after_class: None, or a callable invoked as after_class(class_name, image_dataset, masks, labels, preds, preds_image,
    file_names, details_of_class) once the class's row is computed and before its tensors are released (the dataset is
    the one that was evaluated, details_of_class is details[class_name] or None); None changes nothing.
    bootstrap: None, or dict(R=, seed=0, level=0.95, stratified=False): metrics_eval's keyword for every class, with the
    class's position in image_datasets as class_index -- the interval columns of forward_utils.bootstrap_interval_cols
    in every row and, by bootstrap_average, in the average; details[class]["bootstrap"] holds the replicates.  One
    process only.  None changes nothing."""
    import torch.distributed as dist
    if bootstrap is not None and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise ValueError("evaluate_rows: bootstrap runs in one process (the replicates of a sharded class are not gathered)")
    if bootstrap is not None and details is None:
        details = {}
    if defects is not None and not f1_max:
        raise ValueError("evaluate_rows: defects needs f1_max=True (the regions are those at the pixel F1-max threshold)")
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    rank = dist.get_rank() if world > 1 else 0
    rows = []
    for class_name, image_dataset in image_datasets.items():
        total = len(image_dataset)
        if world > 1:
            b, e = shard_range(total, rank, world)
            image_dataset = torch.utils.data.Subset(image_dataset, list(range(b, e)))
        if len(image_dataset) > 0:
            loader = torch.utils.data.DataLoader(image_dataset, batch_size=batch_size, shuffle=False, **(loader_kwargs or {}))
            bank = {} if support is None else {"support": support[class_name], "support_weight": support_weight}
            nearest = [] if bank and details is not None and return_masks else None
            if nearest is not None:
                bank["nearest"] = nearest
            predict = get_predictions_support if bank else get_predictions
            with torch.no_grad():
                masks, labels, preds, preds_image, file_names = predict(
                    model=model, class_text_embeddings=text_embeddings[class_name], test_loader=loader, device=device,
                    img_size=img_size, dataset=dataset, use_iqm=use_iqm, on_device=device_metrics and world == 1, **bank)
        else:   # more ranks than images of this class
            masks = np.zeros((0, 1, img_size, img_size), np.float32)
            labels, preds_image = np.zeros((0,), np.int64), np.zeros((0,), np.float32)
            preds, file_names, nearest = np.zeros((0, img_size, img_size), np.float32), [], None
        if world > 1:
            gdev = device if dist.get_backend() == "nccl" else None
            masks, labels, preds, preds_image = gather_predictions(
                ((masks != 0).astype(np.uint8), labels.astype(np.int64), preds.astype(np.float32),
                 preds_image.astype(np.float32)), total, device=gdev)
            if device_metrics:
                masks = torch.from_numpy(np.ascontiguousarray(masks)).to(device)
                preds = torch.from_numpy(np.ascontiguousarray(preds)).to(device)
            else:
                masks = masks.astype(np.float32)
        row_of = metrics_eval_device if device_metrics else metrics_eval
        extra = {}
        if f1_max:
            extra["f1_max"] = True
            if defects is not None:
                extra["defects"] = defects
            if details is not None:
                if world > 1:
                    shards = [None] * world
                    dist.all_gather_object(shards, list(file_names))
                    file_names = [name for shard in shards for name in shard]
                scores = preds_image.detach().cpu().numpy() if torch.is_tensor(preds_image) else np.asarray(preds_image)
                extra["details"] = details[class_name] = {
                    "masks": bool(return_masks), "file_names": list(file_names),
                    "labels": [int(v) for v in np.asarray(labels).reshape(-1)],
                    "image scores": [float(v) for v in scores.reshape(len(file_names), -1)[:, 0]] if file_names else []}
                if support is not None and return_masks:
                    details[class_name]["support nearest"] = _support_nearest_pairs(nearest, support[class_name], world)
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
    cols = (TL.NUMERIC_COLS + ([AUPRO_COL] if fpr_limit is not None else []) + (F1_COLS if f1_max else []) +
            (DEFECT_COLS if defects is not None else []))
    avg = {c: float(np.mean([r[c] for r in rows])) for c in cols}
    avg["class name"] = "Average"
    if bootstrap is not None:
        bootstrap_average(avg, [details[r["class name"]]["bootstrap"] for r in rows])
    rows.append(avg)
    return rows


def bootstrap_average(avg: dict, per_class: List[dict]) -> dict:
    """The Average row's intervals: per replicate the mean over the classes of that replicate's values -- every class
    draws with the same seed and R, so replicate r of the average is replicate r of every class -- invalid where any
    class's replicate is; the interval is that of the means, in percent, unrounded like the row's other entries.
    per_class: the details[class]["bootstrap"] dicts.  -> {"valid": mask, column: means} (avg gets the columns)."""
    from forward_utils import BOOTSTRAP_COLS, bootstrap_interval
    valid = np.logical_and.reduce([b["valid"] for b in per_class])
    out = {"valid": valid}
    for col in BOOTSTRAP_COLS:
        out[col] = np.mean([b[col] for b in per_class], axis=0)
        lo, hi = bootstrap_interval(out[col], valid, per_class[0]["level"])
        avg[col + " lo"], avg[col + " hi"] = lo * 100, hi * 100
    return out


def _support_nearest_pairs(nearest, bank, world):
    """per batch, per level int32 [b, P] device indices -> per level int32 [N, P, 2] host arrays of (shot, patch); under
    torch.distributed the shards are joined in rank order.  A bank with an `index` (engine.CoresetBank) holds a part of
    the full bank's rows: the nearest kept row is mapped through index[l] first, so (shot, patch) stay those of the
    full bank."""
    levels = len(bank.rows)
    index = bank.index if "index" in getattr(bank, "_fields", ()) else None     # a plain tuple's .index is a method
    out = []
    for l in range(levels):
        parts = [b[l].cpu().numpy() for b in (nearest or [])]
        idx = np.concatenate(parts, axis=0) if parts else np.zeros((0, bank.patches), np.int32)
        if index is not None:
            idx = index[l].cpu().numpy()[idx]
        out.append(np.stack(np.divmod(idx, bank.patches), axis=-1).astype(np.int32))
    if world > 1:
        import torch.distributed as dist
        shards = [None] * world
        dist.all_gather_object(shards, out)
        out = [np.concatenate([s[l] for s in shards], axis=0) for l in range(levels)]
    return out


def support_banks(model, image_datasets, k: int, device, img_size: int, form=None, support_datasets=None,
                  batch_size: int = 32, coreset=None, coreset_dim=128):
    """The k-shot protocol for every class: -> ({class name: engine.SupportBank}, {class name: evaluated dataset}).
    Without support_datasets the class's first k normal images feed the bank and leave the evaluated set
    (BaseSingleClassDataset.support_split); with them -- datasets of another metadata file, such as MVTec's train/good --
    their first k normal images feed it and the evaluated set stays whole.  Every process that calls this builds the same
    banks: k images per class, no communication.  coreset: None, or the share of every bank's rows that is kept
    (forward_utils.build_support_bank's keyword, with coreset_dim beside it): the banks are engine.CoresetBank then."""
    from forward_utils import build_support_bank
    banks, evaluated = {}, {}
    for class_name, ds in image_datasets.items():
        if support_datasets is None:
            shots, evaluated[class_name] = ds.support_split(k)
        else:
            shots, evaluated[class_name] = support_datasets[class_name].support_split(k)[0], ds
        batches = []
        for b in torch.utils.data.DataLoader(shots, batch_size=batch_size, shuffle=False):
            image = b["image"].to(device)
            batches.append(engine.preprocess(image, img_size) if image.dtype == torch.uint8 else image)
        extra = {} if coreset is None else {"coreset": coreset, "coreset_dim": coreset_dim}
        banks[class_name] = build_support_bank(model, batches, form, **extra)
    return banks, evaluated


def log_coreset(logger, banks):
    """per class and level: the full bank's rows N, the rows kept and the final covering radius as a cosine distance
    (radius2 / 2^29: d^2 = 2 - 2 cos on unit rows, in units of 2^-28)"""
    for class_name, b in banks.items():
        for l, (rows, r2) in enumerate(zip(b.rows, b.radius2)):
            logger.info("coreset %s level %d: N %d, kept %d, covering radius %.6f (cosine distance, dim %d)", class_name, l,
                        b.shots * b.patches, rows.shape[0], float(r2[-1]) / float(1 << 29), b.dim)


def format_table(rows: List[dict]) -> str:
    """test_last.format_table, with the AUPRO column, the two F1-max columns and the bootstrap interval columns behind it
    where the rows carry them"""
    from forward_utils import bootstrap_interval_cols
    table = TL.format_table(rows)
    for col in [AUPRO_COL] + F1_COLS + bootstrap_interval_cols():
        if rows and col in rows[0]:
            extra = [f"{col:>14s}"] + [f"{r[col]:>14.2f}" for r in rows]
            table = "\n".join(line + "  " + cell for line, cell in zip(table.split("\n"), extra))
    return table


def load_adapters(model, save_path: str, logger=None) -> bool:
    """As test_last.load_adapters (reference test_last.py:230-251: optional text adapter, newest image adapter by epoch
    number), then the IQM branch, which the reference never saves: a separate iqm_branch.pth (flat AdaptedCLIP
    state_dict keys) if present, else the "iqm_branch" entry of that newest image_adapter_<epoch>.pth, {module name:
    state_dict} as train.train_image_adapter writes it (train.iqm_branch_state), else the seeded initialisation.
    Logs which source was used."""
    text_file = glob(os.path.join(save_path, "text_adapter.pth"))
    adapt_text = len(text_file) > 0
    if adapt_text:
        ckpt = torch.load(text_file[0], map_location="cpu", weights_only=True)
        model.text_adapter.load_state_dict(ckpt["text_adapter"])
    files = glob(os.path.join(save_path, "image_adapter_*.pth"))
    assert len(files) > 0, "image adapter checkpoint not found"
    files = sorted(files, key=lambda x: int(x.split("_")[-1].split(".")[0]))
    ckpt = torch.load(files[-1], map_location="cpu", weights_only=True)
    model.image_adapter.load_state_dict(ckpt["image_adapter"])
    if logger:
        logger.info("load model from epoch %s", ckpt.get("epoch"))
    iqm_file = os.path.join(save_path, "iqm_branch.pth")
    if os.path.exists(iqm_file):
        sd = torch.load(iqm_file, map_location="cpu", weights_only=True)
        missing, unexpected = model.load_state_dict(sd.get("iqm_branch", sd), strict=False)
        assert not unexpected, unexpected
        source = iqm_file
    elif "iqm_branch" in ckpt:
        import train
        train.load_iqm_branch_state(model, ckpt["iqm_branch"])
        source = f'the "iqm_branch" entry of {files[-1]}'
    else:
        source = None
    if logger:
        if source:
            logger.info("IQM branch weights loaded from %s", source)
        else:
            logger.info("no IQM branch weights in %s: the branch keeps its seeded initialisation", save_path)
    return adapt_text


def build_parser() -> argparse.ArgumentParser:
    """test_last.py's arguments with its defaults (see the notes on the IQM flags there), plus --device_metrics"""
    parser = argparse.ArgumentParser(description="AA-CLIP evaluation on MI355X, metrics on the host or on the GPU")
    parser.add_argument("--model_name", type=str, default="ViT-L-14-336")
    parser.add_argument("--img_size", type=int, default=518)
    parser.add_argument("--relu", action="store_true")
    parser.add_argument("--dataset", type=str, default="MVTec")
    parser.add_argument("--shot", type=int, default=4)
    parser.add_argument("--batch_size", type=int, default=32)
    parser.add_argument("--image_batch_size", type=int, default=32)
    parser.add_argument("--seed", type=int, default=111)
    parser.add_argument("--save_path", type=str, default="ckpt/baseline")
    parser.add_argument("--text_adapt_weight", type=float, default=0.1)
    parser.add_argument("--image_adapt_weight", type=float, default=0.1)
    parser.add_argument("--text_adapt_until", type=int, default=3)
    parser.add_argument("--image_adapt_until", type=int, default=6)
    parser.add_argument("--iqm_hidden_size", type=int, default=768)
    parser.add_argument("--iqm_num_layers", type=int, default=2)
    parser.add_argument("--iqm_num_heads", type=int, default=8)
    parser.add_argument("--iqm_weight", type=float, default=0.7)
    parser.add_argument("--precision", type=str, default="fp16x2", help="fp16x2 (default), fp32, fp16 or bf16")
    parser.add_argument("--device_preprocess", action="store_true", help="resize + normalise on the GPU")
    parser.add_argument("--device_metrics", action="store_true",
                        help="pixel / image AUROC and AP on the GPU (exact: the numbers of the host path) instead of sklearn")
    parser.add_argument("--iqm", choices=["on", "off"], default="on",
                        help="on: maps = 0.6 text + 0.4 IQM like the reference; off: text-only branch")
    return parser


def main(argv=None):
    """The steps of test_last.main with this module's load_adapters and evaluate."""
    return run(build_parser(), argv)


def check_arguments(parser: argparse.ArgumentParser, args) -> None:
    """what this script and eval_aupro.py refuse"""
    aupro = getattr(args, "aupro", None)
    if args.iqm_hidden_size != 768:
        parser.error("--iqm_hidden_size must be 768 (the visual features' width; see test_last.py)")
    if aupro is not None and not 0.0 < aupro <= 1.0:
        parser.error("--aupro takes a false-positive rate in (0, 1]")


Session = collections.namedtuple("Session", "logger device clip_model model adapt_text image_datasets text_embeddings "
                                            "support_datasets")


def open_session(args, name: str, canvas=None, log_lines=()) -> Session:
    """What every script of the tower sets up before it evaluates, once: the seed, <save_path>/test.log with a logger
    called `name` (the `args:` line, then log_lines), the device (and, under WORLD_SIZE > 1, the process group), the CLIP
    model and the AdaptedCLIP around it at --img_size with the adapters of load_adapters, the datasets at `canvas` pixels
    (None: --img_size; eval_tiled.py's frames are larger than the model's side), the text embeddings -- of the adapted
    model where a text adapter was loaded -- and, for --support K with --support_meta, that file's datasets at the canvas
    size (else None).  Arguments that the lower parsers lack count as absent."""
    from dataset import DATA_PATH, BaseSingleClassDataset, get_dataset
    from forward_utils import get_adapted_text_embedding
    from model.adapter import AdaptedCLIP
    from model.clip import create_model
    canvas = args.img_size if canvas is None else canvas
    TL.setup_seed(args.seed)
    os.makedirs(args.save_path, exist_ok=True)
    logger = logging.getLogger(name)
    logging.basicConfig(filename=os.path.join(args.save_path, "test.log"), encoding="utf-8", level=logging.INFO)
    logger.info("args: %s", vars(args))
    for line in log_lines:
        logger.info("%s", line)
    if not torch.cuda.is_available():
        raise RuntimeError("the AA-CLIP HIP path needs an MI355X; there is no CPU fallback")
    local = int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1)
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(os.environ.get("AACLIP_BENCH_BACKEND", "nccl"))
    clip_model = create_model(model_name=args.model_name, img_size=args.img_size, device=device, pretrained="openai",
                              require_pretrained=True, precision=args.precision)
    clip_model.eval()
    model = AdaptedCLIP(clip_model=clip_model, text_adapt_weight=args.text_adapt_weight,
                        image_adapt_weight=args.image_adapt_weight, text_adapt_until=args.text_adapt_until,
                        image_adapt_until=args.image_adapt_until, relu=args.relu,
                        iqm_hidden_size=args.iqm_hidden_size, iqm_num_layers=args.iqm_num_layers,
                        iqm_num_heads=args.iqm_num_heads).to(device)
    model.eval()
    adapt_text = load_adapters(model, args.save_path, logger)
    image_datasets = get_dataset(args.dataset, canvas, None, args.shot, "test", logger=logger,
                                 device_preprocess=args.device_preprocess)
    with torch.no_grad():
        text_embeddings = get_adapted_text_embedding(model if adapt_text else clip_model, args.dataset, device)
    support_datasets = None
    if getattr(args, "support", None) is not None and getattr(args, "support_meta", None):
        support_datasets = {c: BaseSingleClassDataset(DATA_PATH[args.dataset], args.support_meta, canvas, c,
                                                      device_preprocess=args.device_preprocess) for c in image_datasets}
    return Session(logger, device, clip_model, model, adapt_text, image_datasets, text_embeddings, support_datasets)


def run(parser: argparse.ArgumentParser, argv=None, table=None, finish=None):
    """main() for a parser that may carry further arguments: `aupro` (eval_aupro.py), a false-positive rate or None,
    `f1max` (eval_metrics.py), which adds the F1-max columns and logs every class's thresholds, and `defects`
    (eval_defects.py), a minimum area or None, which implies f1max and adds the region-level columns, and `support`
    (eval_support.py), a number of shots or None, with `support_weight`, `support_form` and `support_meta` beside it: the
    banks of support_banks are built after the text embeddings and every class is evaluated with its bank.  table: the
    function that formats the rows (format_table); finish(args, rows, details): called after the evaluation when the
    F1-max path ran."""
    args = parser.parse_args(argv)
    defects = getattr(args, "defects", None)
    aupro, f1_max = getattr(args, "aupro", None), bool(getattr(args, "f1max", False)) or defects is not None
    check_arguments(parser, args)
    session = open_session(args, __name__)
    logger, device, model, image_datasets = session.logger, session.device, session.model, session.image_datasets
    shots, bank = getattr(args, "support", None), {}
    if shots is not None:
        coreset = getattr(args, "support_coreset", None)
        core = {} if coreset is None else {"coreset": coreset, "coreset_dim": getattr(args, "support_coreset_dim", 128)}
        banks, image_datasets = support_banks(model, image_datasets, shots, device, args.img_size,
                                              form=getattr(args, "support_form", None),
                                              support_datasets=session.support_datasets,
                                              batch_size=args.image_batch_size, **core)
        bank = {"support": banks, "support_weight": getattr(args, "support_weight", SUPPORT_WEIGHT)}
        logger.info("support banks: %d shots per class, form %s, weight %s", shots,
                    "fp16" if next(iter(banks.values())).form == engine.SUPPORT_FP16 else "fp32", bank["support_weight"])
        if coreset is not None:
            log_coreset(logger, banks)
    where = (model, image_datasets, session.text_embeddings, device, args.img_size, args.dataset)
    how = dict(batch_size=args.image_batch_size, loader_kwargs={"num_workers": 4, "pin_memory": True}, logger=logger,
               use_iqm=args.iqm == "on", device_metrics=args.device_metrics)
    if f1_max:
        details = {}
        extra = dict(bank) if defects is None else dict(bank, defects=defects)
        rows = evaluate_rows(*where, **how, fpr_limit=aupro, f1_max=True, details=details, **extra)
        for name, d in details.items():
            logger.info("%s: pixel threshold %.9g, image threshold %s (normalised units)", name, d["pixel threshold"],
                        d["image threshold"])
        if finish is not None:
            finish(args, rows, details)
    else:
        rows = (evaluate(*where, **how) if aupro is None and not bank else
                evaluate_rows(*where, **how, fpr_limit=aupro, **bank))
    table = (table or format_table)(rows)
    logger.info("final results:\n%s", table)
    if int(os.environ.get("RANK", "0")) == 0:
        print(table)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        torch.distributed.destroy_process_group()
    return rows


if __name__ == "__main__":
    main()
