#!/usr/bin/env python3
"""Golden vectors of the stage-1 training loss, made by RUNNING THE REFERENCE'S OWN calculate_similarity_map
(test=False) and calculate_seg_loss (reference forward_utils.py:21-108,196-227) with torch autograd on the CPU, in
fp64, on the inputs of tests/seg_loss_cases.py (stubs as in make_golden.py).  Per case it records the loss, its three
terms (the reference's focal_loss / dice_loss objects called the way calculate_seg_loss calls them), the gradient of
the loss with respect to the anchors (fp64), and SEG_ROWS rows per image of its gradient with respect to the patch
features (fp32, to keep the file small).

Usage:  python tests/golden/make_golden_seg_loss.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
from seg_loss_cases import CASES, make_case, seg_rows  # noqa: E402


def main():
    FU = MG._stub_and_import_reference()[4]
    out = {}
    for name, (B, g, S, _kinds, _shared) in CASES.items():
        f, t, mask = make_case(name)
        f.requires_grad_(True)
        t.requires_grad_(True)
        preds = FU.calculate_similarity_map(f, t, S)
        loss = FU.calculate_seg_loss(preds, mask)
        terms = [FU.focal_loss(preds, mask), FU.dice_loss(preds[:, 0, :, :], 1 - mask),
                 FU.dice_loss(preds[:, 1, :, :], mask)]
        loss.backward()
        rows = seg_rows(g * g)
        out[f"{name}.loss"] = np.float64(loss.item())
        out[f"{name}.terms"] = np.array([v.item() for v in terms], dtype=np.float64)
        out[f"{name}.d_anchors"] = t.grad.numpy()
        out[f"{name}.d_seg_rows"] = f.grad[:, rows, :].float().numpy()   # fp32: size
        print(name, loss.item(), [round(v.item(), 6) for v in terms], float(t.grad.norm()), float(f.grad.norm()))
    np.savez_compressed(os.path.join(HERE, "seg_loss.npz"), **out)


if __name__ == "__main__":
    main()
