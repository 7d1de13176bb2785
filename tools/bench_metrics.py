"""Time of one class's pixel / image AUROC and AP: forward_utils.metrics_eval (numpy + sklearn on the host, the default
path of test_last.py) next to forward_utils.metrics_eval_device (csrc/metrics.hip), alternating in one process on the
same synthetic class: N maps of 518 x 518 generated on the device, 3 % positive pixels.  The two rows are compared too.

  host      wall time of metrics_eval on host arrays (the copy of the maps to the host is timed on its own)
  device    wall time and device-event time of metrics_eval_device on the device tensors, result on the host
  split     device-event time between the library entries of the pixel-level call: range, normalise, sort, curve

python tools/bench_metrics.py [--images 64 170] [--rounds 2] [--out profiles/metrics_device_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aa-clip-iqm_amd"))
import forward_utils as FU  # noqa: E402
from aaclip_hip import engine  # noqa: E402

S = 518


def make_class(n_img, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    masks = (torch.rand(n_img, 1, S, S, device=dev, generator=g) < 0.03).to(torch.uint8)
    labels = np.arange(n_img) % 2                  # image labels only enter the N-element image-level pair
    maps = torch.randn(n_img, S, S, device=dev, generator=g) + 1.5 * masks[:, 0].float()
    scores = torch.randn(n_img, device=dev, generator=g) + 1.2 * torch.from_numpy(labels).to(dev).float()
    return masks, labels, maps.contiguous(), scores


def timed_device(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0, a.elapsed_time(b) * 1e-3


def split_times(maps, masks):
    """The pixel-level call of engine.curve_metrics entry by entry, device events between the entries"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    labels = masks.view(-1)
    torch.cuda.synchronize()
    ev[0].record()
    rec, image_max = engine.metrics_range(maps, labels, S * S)
    ev[1].record()
    norm = engine.metrics_normalise(maps.view(-1), rec)
    engine.metrics_normalise(image_max, rec, out=image_max)
    ev[2].record()
    keys, labels_sorted, _ = engine.metrics_sort(norm, labels, True)
    ev[3].record()
    engine.metrics_curve(keys, labels_sorted, True)
    ev[4].record()
    torch.cuda.synchronize()
    return {k: ev[i].elapsed_time(ev[i + 1]) * 1e-3 for i, k in enumerate(["range_s", "normalise_s", "sort_s", "curve_s"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[64, 170])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_device_timing.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    record = {"device": torch.cuda.get_device_name(0), "map_size": S, "positive_pixel_share": 0.03, "rounds": args.rounds,
              "classes": []}
    for n_img in args.images:
        masks, labels, maps, scores = make_class(n_img, dev, seed=n_img)
        FU.metrics_eval_device(masks, labels, maps, scores, "warm-up", "Industrial")        # sizes the workspace
        host_s, d2h_s, dev_wall, dev_event, splits = [], [], [], [], []
        rows_equal = True
        for r in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h_masks, h_maps, h_scores = masks.float().cpu().numpy(), maps.cpu().numpy(), scores.cpu().numpy()
            d2h_s.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            row_host = FU.metrics_eval(h_masks, labels, h_maps, h_scores, f"n{n_img}", "Industrial")
            host_s.append(time.perf_counter() - t0)
            del h_masks, h_maps
            print(f"N={n_img} round {r}: host {host_s[-1]:.2f} s (+ {d2h_s[-1]:.2f} s copy to the host)", flush=True)
            for _ in range(3):
                row_dev, wall, event = timed_device(
                    lambda: FU.metrics_eval_device(masks, labels, maps, scores, f"n{n_img}", "Industrial"))
                dev_wall.append(wall)
                dev_event.append(event)
                rows_equal = rows_equal and row_dev == row_host
            splits.append(split_times(maps, masks))
            print(f"N={n_img} round {r}: device wall {dev_wall[-3:]} s, events {dev_event[-3:]} s, rows equal: "
                  f"{row_dev == row_host}; {splits[-1]}", flush=True)
        exact = engine.curve_metrics(maps, masks, per_image=S * S)
        record["classes"].append({
            "images": n_img, "pixels": n_img * S * S, "tie_groups": exact.groups, "positives": exact.P,
            "pixel_auroc": exact.auroc, "pixel_ap": exact.ap, "row": row_dev, "rows_equal_host": rows_equal,
            "host_metrics_eval_wall_s": host_s, "host_copy_wall_s": d2h_s,
            "device_metrics_eval_wall_s": dev_wall, "device_metrics_eval_event_s": dev_event,
            "device_entries_event_s": splits,
            "host_over_device_wall": float(np.median(host_s) / np.median(dev_wall))})
        del masks, maps, scores
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print(json.dumps(record))


if __name__ == "__main__":
    main()
