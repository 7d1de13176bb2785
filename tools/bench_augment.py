"""Per-sample time of the train-time input work: engine.train_preprocess on raw uint8 frames (upload included) next to
dataset.train_transform on one host core with one torch thread, which is what a DataLoader worker runs.  Both apply the
same drawn numbers with every step switched on.  python tools/bench_augment.py"""
import os
import sys
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aa-clip-iqm_amd"))
import dataset as D  # noqa: E402
from aaclip_hip import engine  # noqa: E402


def main():
    dev = torch.device("cuda:0")
    S, B = 518, 16
    rng = np.random.default_rng(0)
    for (H, W) in [(1024, 1024), (518, 518)]:
        frames = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).pin_memory()
        masks = torch.from_numpy((rng.random((B, H, W)) < 0.1).astype(np.uint8) * 255).pin_memory()
        normal = torch.zeros(B, dtype=torch.int32)
        params = D.draw_augment_params(torch.Generator().manual_seed(0), B, S, False)
        params["color_apply"].fill_(7)
        params["flags"].fill_(15)

        def step():
            return engine.train_preprocess(frames.to(dev, non_blocking=True), masks.to(dev, non_blocking=True),
                                           normal.to(dev), params, S)
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        n, runs = 300, []
        for _ in range(3):                       # three windows of 300 batches each: the spread is part of the figure
            t0 = time.perf_counter()
            for _ in range(n):
                step()
            torch.cuda.synchronize()
            runs.append((time.perf_counter() - t0) / n / B * 1e3)
        dev_ms = sorted(runs)[1]
        torch.set_num_threads(1)
        imgs = [Image.fromarray(frames[b].numpy()) for b in range(4)]
        mks = [Image.fromarray(masks[b].numpy()) for b in range(4)]
        t0 = time.perf_counter()
        for b in range(4):
            D.train_transform(imgs[b], mks[b], params, S, b)
        host_ms = (time.perf_counter() - t0) / 4 * 1e3
        print(f"{H}x{W} -> {S}, batch {B}: device {dev_ms:.3f} ms/sample (median of {[round(r, 3) for r in runs]}; pinned "
              f"upload + 6 kernels, host clock around {n} batches ending in a synchronise); host {host_ms:.1f} ms/sample "
              f"on one core", flush=True)


if __name__ == "__main__":
    main()
