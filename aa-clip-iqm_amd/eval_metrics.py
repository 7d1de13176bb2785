"""eval_aupro.py with the F1-max columns and the operating point: its arguments and steps, plus

  --f1max    add "pixel F1-max" and "image F1-max", the best F1 over every distinct threshold of every class
             (forward_utils.f1max_eval on the host; with --device_metrics engine.f1max_metrics, from the one sort that
             serves AUROC / AP), and log every class's thresholds, in the normalised units metrics_eval works in:
             predicted = normalised score >= threshold

Without --f1max it prints exactly what eval_aupro.py prints.  evaluate(..., f1_max=True, return_masks=True) also hands
back every class's predicted uint8 masks at its pixel operating point -- on the GPU, from engine.metrics_threshold, with
--device_metrics / device_metrics=True.

python eval_metrics.py --save_path ... [--device_metrics] [--aupro [LIMIT]] [--f1max] [every argument of test_last.py]
"""
from __future__ import annotations

import argparse

import eval_aupro as EA
import eval_last as EL


def evaluate(model, image_datasets, text_embeddings, device, img_size: int, dataset: str, batch_size: int = 32,
             loader_kwargs=None, logger=None, use_iqm: bool = True, device_metrics: bool = False, aupro_limit=None,
             f1_max: bool = False, return_masks: bool = False):
    """eval_aupro.evaluate; f1_max adds "pixel F1-max" and "image F1-max" to every row and to the average, on either
    metrics path.  return_masks (needs f1_max): -> (rows, details) with details[class name] = {"pixel threshold",
    "image threshold" (None where the class has one image label only), "masks": the uint8 predicted masks in the maps'
    shape, normalised map >= pixel threshold -- a device tensor when device_metrics}."""
    how = dict(batch_size=batch_size, loader_kwargs=loader_kwargs, logger=logger, use_iqm=use_iqm,
               device_metrics=device_metrics)
    where = (model, image_datasets, text_embeddings, device, img_size, dataset)
    if not f1_max:
        if return_masks:
            raise ValueError("eval_metrics.evaluate: return_masks needs f1_max=True (the masks are those of its threshold)")
        return EA.evaluate(*where, **how, aupro_limit=aupro_limit)
    details = {}
    rows = EL.evaluate_rows(*where, **how, fpr_limit=aupro_limit, f1_max=True, details=details, return_masks=return_masks)
    return (rows, details) if return_masks else rows


def build_parser() -> argparse.ArgumentParser:
    parser = EA.build_parser()
    parser.add_argument("--f1max", action="store_true",
                        help="add the pixel / image F1-max columns (the best F1 over every threshold, exact on either "
                             "metrics path) and log every class's thresholds")
    return parser


def main(argv=None):
    return EL.run(build_parser(), argv)


if __name__ == "__main__":
    main()
