"""eval_defects.py with a few-shot support bank: its arguments and steps, plus

  --support K            use K known-good images of every class without training: the model's seg tokens of those images form
                         a bank per tap level, and every test patch's cosine distance to its nearest bank patch
                         (csrc/support.hip: the cosines stay in MFMA accumulators, one maximum per row is written) is
                         blurred, upsampled and summed over the levels like the text map and added to it, times
                         --support_weight, before the IQM fusion.  The K images are the class's first K normal images of
                         the metadata file, in file order, and they are REMOVED from the evaluated set.
  --support_weight W     default 50: the text map is 50 * (cos_1 - cos_0) + 0.5 per level, so one unit of cosine distance to
                         the bank weighs as much as one unit of anchor-cosine difference.  Derived, not tuned.
  --support_form F       fp16 (both operands rounded to fp16 on the MFMA, |error| < 1.1e-3 per cosine) or fp32; default:
                         fp32 for --precision fp32, fp16 otherwise
  --support_meta FILE    a jsonl in the metadata format whose label-0 entries of every class feed the bank instead, e.g.
                         MVTec's train/good; nothing is removed from the test set then

Without --support it prints exactly what eval_defects.py prints.  evaluate(..., support=K) is the function form.

python eval_support.py --save_path ... [--device_metrics] [--support K] [--support_weight W] [--support_form fp16|fp32]
                       [--support_meta FILE] [every argument of eval_defects.py]
"""
from __future__ import annotations

import argparse

import eval_defects as ED
from forward_utils import SUPPORT_WEIGHT


def evaluate(model, image_datasets, text_embeddings, device, img_size: int, dataset: str, batch_size: int = 32,
             loader_kwargs=None, logger=None, use_iqm: bool = True, device_metrics: bool = False, aupro_limit=None,
             f1_max: bool = False, return_masks: bool = False, defects=None, save_path=None, support=None,
             support_weight: float = SUPPORT_WEIGHT, support_form=None, support_datasets=None):
    """eval_defects.evaluate; support: a number of shots K builds every class's bank (eval_last.support_banks: from the
    class's first K normal images, which leave the evaluated set, or from support_datasets) and evaluates with it.
    return_masks (with f1_max or defects): details[class]["support nearest"] holds per tap level the (shot, patch) of the
    nearest bank patch of every evaluated patch.  support=None is eval_defects.evaluate."""
    where = (model, image_datasets, text_embeddings, device, img_size, dataset)
    how = dict(batch_size=batch_size, loader_kwargs=loader_kwargs, logger=logger, use_iqm=use_iqm,
               device_metrics=device_metrics)
    if support is None:
        return ED.evaluate(*where, **how, aupro_limit=aupro_limit, f1_max=f1_max, return_masks=return_masks, defects=defects,
                           save_path=save_path)
    f1 = f1_max or defects is not None
    rows, details = ED.evaluate_details(*where, **how, aupro_limit=aupro_limit, f1_max=f1, return_masks=return_masks,
                                        defects=defects, save_path=save_path, support=support,
                                        support_weight=support_weight, support_form=support_form,
                                        support_datasets=support_datasets)
    return (rows, details) if return_masks and f1 else rows


def build_parser() -> argparse.ArgumentParser:
    parser = ED.build_parser()
    parser.add_argument("--support", type=int, default=None, metavar="K",
                        help="few-shot support bank from K normal images per class (removed from the evaluated set)")
    parser.add_argument("--support_weight", type=float, default=SUPPORT_WEIGHT,
                        help="weight of the support distance in the text map (derived default 50, not tuned)")
    parser.add_argument("--support_form", choices=["fp16", "fp32"], default=None,
                        help="arithmetic of the nearest-patch search; default fp32 for --precision fp32, else fp16")
    parser.add_argument("--support_meta", type=str, default=None, metavar="FILE",
                        help="metadata jsonl whose label-0 entries feed the banks instead (nothing leaves the test set)")
    return parser


def check_arguments(parser: argparse.ArgumentParser, args) -> None:
    if args.support is not None and args.support < 1:
        parser.error("--support takes at least 1 shot")


def run(parser: argparse.ArgumentParser, argv=None):
    """Without --support: eval_defects.run.  With it: the same steps with the banks built after the text embeddings
    (eval_last.run reads the support arguments)."""
    args = parser.parse_args(argv)
    if args.support is None and args.support_meta is not None:
        parser.error("--support_meta needs --support K")
    check_arguments(parser, args)
    return ED.run(parser, argv)


def main(argv=None):
    return run(build_parser(), argv)


if __name__ == "__main__":
    main()
