"""eval_last.py with the per-region overlap column: its arguments and steps, plus

  --aupro [LIMIT]    add "pixel AUPRO", the per-region overlap (PRO) curve of every class integrated up to the
                     false-positive rate LIMIT (0.3 when given without a value) and divided by it, over every distinct
                     score: forward_utils.pro_eval on the host, pro_eval_device (csrc/regions.hip) with --device_metrics

Without --aupro it prints exactly what eval_last.py prints.  eval_last.py's own arguments and evaluate() stay
test_last.py's plus --device_metrics; the loop with the column is eval_last.evaluate_rows(fpr_limit=...), also reached as
evaluate(..., aupro_limit=...) here.

python eval_aupro.py --save_path ... [--device_metrics] [--aupro [LIMIT]] [every argument of test_last.py]
"""
from __future__ import annotations

import argparse

import eval_last as EL

AUPRO_DEFAULT_LIMIT = 0.3


def evaluate(model, image_datasets, text_embeddings, device, img_size: int, dataset: str, batch_size: int = 32,
             loader_kwargs=None, logger=None, use_iqm: bool = True, device_metrics: bool = False, aupro_limit=None):
    """eval_last.evaluate; aupro_limit: a false-positive rate in (0, 1] adds "pixel AUPRO" to every row and to the
    average, on either metrics path; None returns eval_last.evaluate's rows"""
    how = dict(batch_size=batch_size, loader_kwargs=loader_kwargs, logger=logger, use_iqm=use_iqm,
               device_metrics=device_metrics)
    where = (model, image_datasets, text_embeddings, device, img_size, dataset)
    return EL.evaluate(*where, **how) if aupro_limit is None else EL.evaluate_rows(*where, **how, fpr_limit=aupro_limit)


def build_parser() -> argparse.ArgumentParser:
    parser = EL.build_parser()
    parser.add_argument("--aupro", type=float, nargs="?", const=AUPRO_DEFAULT_LIMIT, default=None, metavar="LIMIT",
                        help="add the pixel AUPRO column: the per-region overlap curve integrated up to the "
                             "false-positive rate LIMIT (0.3 when given without a value); exact on either metrics path")
    return parser


def main(argv=None):
    return EL.run(build_parser(), argv)


if __name__ == "__main__":
    main()
