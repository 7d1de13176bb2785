"""eval_metrics.py with the defect instances at the operating point: its arguments and steps, plus

  --defects [MIN_AREA]   implies --f1max.  At every class's pixel F1-max threshold the predicted masks are split into their
                         connected regions (8-connectivity), regions of fewer than MIN_AREA pixels (1 when given without a
                         value) are dropped, and every region is listed with its box, area, peak score and position and
                         whether it touches ground truth: forward_utils.defects_eval on the host, with --device_metrics
                         engine.defects_at_threshold (csrc/region_table.hip), where maps, masks, threshold and labelling
                         never leave the GPU.  Adds the columns "region recall", "region precision" and "false regions /
                         image" to the table and the average, and writes <save_path>/defects/<dataset>/<class>.jsonl, one
                         line per image:
                           {"file_name", "label", "image_score",
                            "defects": [{"bbox": [x0, y0, x1, y1], "area", "peak", "peak_xy": [x, y], "hit"}, ...]}
                         with the defects in canonical order (by first pixel, row-major), boxes x1 / y1 exclusive, the
                         peak in the normalised units of the thresholds.  Rank 0 writes.

Without --defects it prints exactly what eval_metrics.py prints.  evaluate(..., defects=MIN_AREA) is the function form.
evaluate_details is the evaluation that the scripts from eval_support.py up share: banks, evaluate_rows, these files.

python eval_defects.py --save_path ... [--device_metrics] [--aupro [LIMIT]] [--f1max] [--defects [MIN_AREA]] [...]
"""
from __future__ import annotations

import argparse
import json
import os
from typing import Dict, List

import eval_last as EL
import eval_metrics as EM
from forward_utils import DEFECT_COLS, SUPPORT_WEIGHT

DEFECTS_DEFAULT_MIN_AREA = 1


def defect_lines(details: dict) -> List[str]:
    """One class's details (eval_last.evaluate_rows with defects) -> its JSON lines, one per image"""
    lines = []
    for name, label, score, regions in zip(details["file_names"], details["labels"], details["image scores"],
                                           details["defects"]):
        lines.append(json.dumps({
            "file_name": name, "label": label, "image_score": score,
            "defects": [{"bbox": [r["x0"], r["y0"], r["x1"], r["y1"]], "area": r["area"], "peak": r["peak"],
                         "peak_xy": [r["peak_x"], r["peak_y"]], "hit": r["overlap"] > 0} for r in regions]}))
    return lines


def write_defects(save_path: str, dataset: str, details: Dict[str, dict]) -> List[str]:
    """<save_path>/defects/<dataset>/<class>.jsonl for every class of `details`; -> the paths written"""
    folder = os.path.join(save_path, "defects", dataset)
    os.makedirs(folder, exist_ok=True)
    paths = []
    for class_name, d in details.items():
        paths.append(os.path.join(folder, f"{class_name}.jsonl"))
        with open(paths[-1], "w", encoding="utf-8") as f:
            f.write("".join(line + "\n" for line in defect_lines(d)))
    return paths


def evaluate(model, image_datasets, text_embeddings, device, img_size: int, dataset: str, batch_size: int = 32,
             loader_kwargs=None, logger=None, use_iqm: bool = True, device_metrics: bool = False, aupro_limit=None,
             f1_max: bool = False, return_masks: bool = False, defects=None, save_path=None):
    """eval_metrics.evaluate; defects: a min_area >= 1 (implies f1_max) adds forward_utils.DEFECT_COLS to every row and
    to the average, on either metrics path, and with save_path writes the .jsonl files of write_defects.  return_masks:
    -> (rows, details); details[class name] then holds "defects" (the per-image lists), the unfiltered "masks" and the
    filtered "kept masks" beside the thresholds.  defects=None is eval_metrics.evaluate."""
    how = dict(batch_size=batch_size, loader_kwargs=loader_kwargs, logger=logger, use_iqm=use_iqm,
               device_metrics=device_metrics)
    where = (model, image_datasets, text_embeddings, device, img_size, dataset)
    if defects is None:
        return EM.evaluate(*where, **how, aupro_limit=aupro_limit, f1_max=f1_max, return_masks=return_masks)
    rows, details = evaluate_details(*where, **how, aupro_limit=aupro_limit, f1_max=True, return_masks=return_masks,
                                     defects=defects, save_path=save_path)
    return (rows, details) if return_masks else rows


def evaluate_details(model, image_datasets, text_embeddings, device, img_size: int, dataset: str, batch_size: int = 32,
                     loader_kwargs=None, logger=None, use_iqm: bool = True, device_metrics: bool = False, aupro_limit=None,
                     f1_max: bool = False, return_masks: bool = False, defects=None, save_path=None, support=None,
                     support_weight: float = SUPPORT_WEIGHT, support_form=None, support_datasets=None, coreset=None,
                     coreset_dim: int = 128, bootstrap=None, after_class=None):
    """The evaluation behind every script from this one up, at the model's own size (eval_tiled.evaluate_details is its
    twin over tiles): the banks where support=K asks for them (eval_last.support_banks, reduced by coreset, which is
    logged), eval_last.evaluate_rows -- defects needs f1_max=True; bootstrap and after_class are its keywords -- and the
    .jsonl files of write_defects where defects and save_path ask for them, written by rank 0.  -> (rows, details),
    details None without f1_max and without bootstrap."""
    if coreset is not None and support is None:
        raise ValueError("evaluate: coreset needs support=K")
    banks = None
    if support is not None:
        core = {} if coreset is None else {"coreset": coreset, "coreset_dim": coreset_dim}
        banks, image_datasets = EL.support_banks(model, image_datasets, support, device, img_size, form=support_form,
                                                 support_datasets=support_datasets, batch_size=batch_size, **core)
        if logger and coreset is not None:
            EL.log_coreset(logger, banks)
    details = {} if f1_max or bootstrap is not None else None
    rows = EL.evaluate_rows(model, image_datasets, text_embeddings, device, img_size, dataset, batch_size=batch_size,
                            loader_kwargs=loader_kwargs, logger=logger, use_iqm=use_iqm, device_metrics=device_metrics,
                            fpr_limit=aupro_limit, f1_max=f1_max, details=details, return_masks=return_masks,
                            defects=defects, support=banks, support_weight=support_weight, bootstrap=bootstrap,
                            after_class=after_class)
    write_defects_of(defects, save_path, dataset, details)
    return rows, details


def write_defects_of(defects, save_path, dataset: str, details) -> None:
    """write_defects where the evaluation asked for defects and has a save_path, in the process of rank 0"""
    if defects is not None and save_path is not None and int(os.environ.get("RANK", "0")) == 0:
        write_defects(save_path, dataset, details)


def format_table(rows: List[dict]) -> str:
    """eval_last.format_table, with the three region-level columns behind it where the rows carry them"""
    table = EL.format_table(rows)
    for col in DEFECT_COLS:
        if rows and col in rows[0]:
            width = max(14, len(col))
            extra = [f"{col:>{width}s}"] + [f"{r[col]:>{width}.4f}" for r in rows]
            table = "\n".join(line + "  " + cell for line, cell in zip(table.split("\n"), extra))
    return table


def build_parser() -> argparse.ArgumentParser:
    parser = EM.build_parser()
    parser.add_argument("--defects", type=int, nargs="?", const=DEFECTS_DEFAULT_MIN_AREA, default=None, metavar="MIN_AREA",
                        help="list the defect instances at every class's pixel F1-max threshold (implies --f1max): regions "
                             "of at least MIN_AREA pixels (1 when given without a value); adds the region-level columns "
                             "and writes <save_path>/defects/<dataset>/<class>.jsonl")
    return parser


def check_arguments(parser: argparse.ArgumentParser, args) -> None:
    if args.defects is not None and args.defects < 1:
        parser.error("--defects takes a minimum area of at least 1 pixel")


def log_table(logger, rows) -> None:
    """this module's table into the log and onto the terminal: how the scripts above this one end"""
    table = format_table(rows)
    logger.info("final results:\n%s", table)
    print(table)


def run(parser: argparse.ArgumentParser, argv=None):
    """Without --defects: eval_last.run, which is what eval_metrics.py runs.  With it: the same steps with the regions
    asked for, this module's table, and the .jsonl files written by rank 0."""
    args = parser.parse_args(argv)
    if args.defects is None:
        return EL.run(parser, argv)
    check_arguments(parser, args)
    return EL.run(parser, argv, table=format_table,
                  finish=lambda args, rows, details: write_defects_of(args.defects, args.save_path, args.dataset, details))


def main(argv=None):
    return run(build_parser(), argv)


if __name__ == "__main__":
    main()
