"""eval_support.py with a coreset of the support bank: its arguments and steps, plus

  --support_coreset R        keep the share R (0 < R <= 1) of every class's bank rows, chosen by greedy k-center selection
                             on the GPU (csrc/coreset.hip: the row farthest from everything picked so far, in exact
                             integer arithmetic on rows quantised to int16 -- the same picks on every run), and search
                             only those.  The search cost is linear in the bank's rows, so a bank of a class's whole
                             train/good (--support_meta) costs at R = 0.1 what a tenth of its images would.
  --support_coreset_dim D    default 128: the selection runs on the rows projected to D dimensions by a seeded Gaussian
                             matrix and re-normalised (D a multiple of 128); 0 selects on the rows themselves.  The kept
                             rows are always the original ones.

--support_coreset needs --support K.  Without --support_coreset it prints exactly what eval_support.py prints.
evaluate(..., coreset=R, coreset_dim=D) is the function form.  The log holds, per class and level, the bank's rows, the
rows kept and the final covering radius as a cosine distance.

python eval_coreset.py --save_path ... --support K [--support_meta FILE] [--support_coreset R] [--support_coreset_dim D]
                       [every argument of eval_support.py]
"""
from __future__ import annotations

import argparse

import eval_defects as ED
import eval_support as ES
from forward_utils import SUPPORT_WEIGHT


def evaluate(model, image_datasets, text_embeddings, device, img_size: int, dataset: str, batch_size: int = 32,
             loader_kwargs=None, logger=None, use_iqm: bool = True, device_metrics: bool = False, aupro_limit=None,
             f1_max: bool = False, return_masks: bool = False, defects=None, save_path=None, support=None,
             support_weight: float = SUPPORT_WEIGHT, support_form=None, support_datasets=None, coreset=None,
             coreset_dim: int = 128):
    """eval_support.evaluate; coreset: the share of every bank's rows that is kept (eval_last.support_banks' keyword, with
    coreset_dim beside it).  With return_masks, details[class]["support nearest"] keeps its meaning: (shot, patch) of the
    FULL bank.  coreset=None is eval_support.evaluate."""
    where = (model, image_datasets, text_embeddings, device, img_size, dataset)
    how = dict(batch_size=batch_size, loader_kwargs=loader_kwargs, logger=logger, use_iqm=use_iqm,
               device_metrics=device_metrics, aupro_limit=aupro_limit, f1_max=f1_max, return_masks=return_masks,
               defects=defects, save_path=save_path)
    if coreset is None:
        return ES.evaluate(*where, **how, support=support, support_weight=support_weight, support_form=support_form,
                           support_datasets=support_datasets)
    f1 = f1_max or defects is not None
    rows, details = ED.evaluate_details(*where, **dict(how, f1_max=f1), support=support, support_weight=support_weight,
                                        support_form=support_form, support_datasets=support_datasets, coreset=coreset,
                                        coreset_dim=coreset_dim)
    return (rows, details) if return_masks and f1 else rows


def build_parser() -> argparse.ArgumentParser:
    parser = ES.build_parser()
    parser.add_argument("--support_coreset", type=float, default=None, metavar="R",
                        help="keep the share R in (0, 1] of every bank's rows (greedy k-center selection on the GPU)")
    parser.add_argument("--support_coreset_dim", type=int, default=128, metavar="D",
                        help="select on rows projected to D dimensions (a multiple of 128); 0: on the rows themselves")
    return parser


def check_arguments(parser: argparse.ArgumentParser, args) -> None:
    if args.support_coreset is not None:
        if not 0.0 < args.support_coreset <= 1.0:
            parser.error("--support_coreset takes a share in (0, 1]")
        if args.support_coreset_dim < 0 or args.support_coreset_dim % 128:
            parser.error("--support_coreset_dim takes 0 or a multiple of 128")


def run(parser: argparse.ArgumentParser, argv=None):
    """Without --support_coreset: eval_support.run.  With it: the same steps, the banks reduced to their coresets
    (eval_last.run reads the coreset arguments)."""
    args = parser.parse_args(argv)
    if args.support_coreset is not None and args.support is None:
        parser.error("--support_coreset needs --support K")
    check_arguments(parser, args)
    return ES.run(parser, argv)


def main(argv=None):
    return run(build_parser(), argv)


if __name__ == "__main__":
    main()
