#!/usr/bin/env python
"""Interval of the DIFFERENCE between two evaluations of the same images, from their bootstrap replicates.

  python tools/bootstrap_diff.py A B [--level 0.95]

A and B are the folders <save_path>/bootstrap/<dataset>/ that eval_bootstrap.py --bootstrap R writes (one <class>.npz per
class and Average.npz).  Both runs must have drawn the same replicates: the same seed, R, image count and stratification
per class, or the tool refuses.  Replicate r of A and replicate r of B then resample the same images, so B[r] - A[r] is
a replicate of the difference; the interval is numpy's default quantiles (1 - level) / 2 and (1 + level) / 2 over the
replicates valid in both.  An interval that excludes 0 says that the difference is larger than the sampling noise of the
class.  Pure numpy; values in percent, like the tables.
"""
import argparse
import os
import sys

import numpy as np

COLUMNS = (("pixel AUC", "pixel_auc"), ("pixel AP", "pixel_ap"), ("image AUC", "image_auc"), ("image AP", "image_ap"))
SAME = ("seed", "R", "images", "stratified")


def load_tree(folder):
    """-> {class name: dict of arrays} of every .npz of the folder"""
    if not os.path.isdir(folder):
        raise ValueError(f"{folder}: no such folder")
    out = {}
    for name in sorted(os.listdir(folder)):
        if name.endswith(".npz"):
            with np.load(os.path.join(folder, name)) as z:
                out[name[:-4]] = {k: z[k] for k in z.files}
    if not out:
        raise ValueError(f"{folder}: no .npz files")
    return out


def diff_rows(a, b, level=0.95):
    """a, b: load_tree's dicts -> rows {class name, and per column: "<column> diff", "... lo", "... hi"}, Average last.
    ValueError where the two trees do not hold the same classes or did not draw the same replicates."""
    if not 0.0 < level < 1.0:
        raise ValueError(f"level must lie in (0, 1), got {level}")
    if set(a) != set(b):
        raise ValueError(f"the trees hold different classes: {sorted(set(a) ^ set(b))}")
    rows = []
    for name in sorted(a, key=lambda c: (c == "Average", c)):
        x, y = a[name], b[name]
        for key in SAME:
            if int(x[key]) != int(y[key]):
                raise ValueError(f"{name}: {key} differs ({int(x[key])} against {int(y[key])}): the two runs did not draw "
                                 "the same replicates")
        valid = x["valid"].astype(bool) & y["valid"].astype(bool)
        if not valid.any():
            raise ValueError(f"{name}: no replicate is valid in both runs")
        row = {"class name": name, "replicates": int(valid.sum())}
        for i, (col, key) in enumerate(COLUMNS):
            d = (y[key][valid] - x[key][valid]) * 100.0
            lo, hi = np.quantile(d, [(1.0 - level) / 2.0, (1.0 + level) / 2.0])
            row[col + " diff"] = float(y["point"][i] - x["point"][i])
            row[col + " lo"], row[col + " hi"] = float(lo), float(hi)
        rows.append(row)
    return rows


def format_rows(rows):
    head = f"{'class name':>16s}  {'replicates':>10s}" + "".join(f"  {col + ' B-A [lo, hi]':>32s}" for col, _ in COLUMNS)
    lines = [head]
    for r in rows:
        cells = "".join(f"  {r[c + ' diff']:>+9.2f} [{r[c + ' lo']:>+8.2f}, {r[c + ' hi']:>+8.2f}]" + " " * 1 for c, _ in COLUMNS)
        lines.append(f"{r['class name']:>16s}  {r['replicates']:>10d}{cells}")
    return "\n".join(lines)


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("A")
    parser.add_argument("B")
    parser.add_argument("--level", type=float, default=0.95)
    args = parser.parse_args(argv)
    try:
        rows = diff_rows(load_tree(args.A), load_tree(args.B), args.level)
    except ValueError as e:
        print(f"bootstrap_diff: {e}", file=sys.stderr)
        return 2
    print(format_rows(rows))
    return 0


if __name__ == "__main__":
    sys.exit(main())
