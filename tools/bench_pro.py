"""Time of one class's pixel AUPRO: forward_utils.pro_eval (numpy + scipy.ndimage.label on the host) next to
forward_utils.pro_eval_device (csrc/regions.hip), alternating in one process on the same synthetic class: N maps of
518 x 518 generated on the device, three rectangular defects per image.  The two values are compared too.

  host      wall time of pro_eval on host arrays (the copy of the maps to the host is timed on its own)
  device    wall time and device-event time of pro_eval_device on the device tensors, result on the host
  split     device-event time between the library entries: regions, range + normalise, pair sort, PRO curve
  row       wall time of metrics_eval_device with and without fpr_limit on the same class: what --aupro adds to
            eval_aupro.py --device_metrics

python tools/bench_pro.py [--images 64 170] [--rounds 2] [--out profiles/pro_device_timing.json]"""
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
LIMIT = 0.3


def make_class(n_img, dev, seed):
    rng = np.random.default_rng(seed)
    masks = np.zeros((n_img, 1, S, S), np.uint8)
    for k in range(n_img):
        for _ in range(3):
            h, w = rng.integers(4, 90, size=2)
            y, x = rng.integers(0, S - h), rng.integers(0, S - w)
            masks[k, 0, y:y + h, x:x + w] = 1
    masks = torch.from_numpy(masks).to(dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    labels = np.arange(n_img) % 2
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
    """engine.pro_metrics entry by entry, device events between the entries"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    torch.cuda.synchronize()
    ev[0].record()
    _, area, regions_record = engine.metrics_regions(masks[:, 0])
    ev[1].record()
    rng, _ = engine.metrics_range(maps)
    norm = engine.metrics_normalise(maps.view(-1), rng)
    ev[2].record()
    keys, areas_sorted = engine.metrics_sort_pairs(norm, area)
    ev[3].record()
    engine.metrics_pro_curve(keys, areas_sorted, regions_record, LIMIT)
    ev[4].record()
    torch.cuda.synchronize()
    names = ["regions_s", "range_normalise_s", "sort_pairs_s", "pro_curve_s"]
    return {k: ev[i].elapsed_time(ev[i + 1]) * 1e-3 for i, k in enumerate(names)}


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "all": [float(x) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[64, 170])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pro_device_timing.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    record = {"device": torch.cuda.get_device_name(0), "map_size": S, "fpr_limit": LIMIT, "defects_per_image": 3,
              "rounds": args.rounds, "classes": []}
    for n_img in args.images:
        masks, labels, maps, scores = make_class(n_img, dev, seed=n_img)
        FU.metrics_eval_device(masks, labels, maps, scores, "warm-up", "Industrial", fpr_limit=LIMIT)   # sizes the workspace
        host_s, d2h_s, dev_wall, dev_event, splits, row_plain, row_aupro, diffs = [], [], [], [], [], [], [], []
        for r in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h_masks, h_maps = masks.cpu().numpy(), maps.cpu().numpy()
            d2h_s.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            host = FU.pro_eval(h_masks, h_maps, fpr_limit=LIMIT)
            host_s.append(time.perf_counter() - t0)
            del h_masks, h_maps
            print(f"N={n_img} round {r}: host {host_s[-1]:.2f} s (+ {d2h_s[-1]:.2f} s copy to the host)", flush=True)
            for _ in range(3):
                got, wall, event = timed_device(lambda: FU.pro_eval_device(masks, maps, fpr_limit=LIMIT))
                dev_wall.append(wall)
                dev_event.append(event)
                diffs.append(abs(got - host))
                _, wall, _ = timed_device(lambda: FU.metrics_eval_device(masks, labels, maps, scores, "c", "Industrial"))
                row_plain.append(wall)
                row, wall, _ = timed_device(
                    lambda: FU.metrics_eval_device(masks, labels, maps, scores, "c", "Industrial", fpr_limit=LIMIT))
                row_aupro.append(wall)
            splits.append(split_times(maps, masks))
            print(f"N={n_img} round {r}: device wall {dev_wall[-3:]} s, events {dev_event[-3:]} s, |device - host| "
                  f"{max(diffs[-3:]):.2e}; {splits[-1]}; row {row_plain[-3:]} -> with AUPRO {row_aupro[-3:]}", flush=True)
        exact = engine.pro_metrics(maps, masks[:, 0], fpr_limit=LIMIT)
        record["classes"].append({
            "images": n_img, "pixels": n_img * S * S, "regions": exact.regions, "normal_pixels": exact.normal,
            "tie_groups": exact.groups, "aupro_device": exact.aupro, "aupro_host": host, "max_abs_diff": float(max(diffs)),
            "row": row, "host_pro_eval_wall_s": spread(host_s), "host_copy_wall_s": spread(d2h_s),
            "device_pro_eval_wall_s": spread(dev_wall), "device_pro_eval_event_s": spread(dev_event),
            "device_entries_event_s": splits,
            "regions_share_of_device_event": float(np.median([s["regions_s"] for s in splits]) / np.median(dev_event)),
            "metrics_eval_device_wall_s": spread(row_plain), "metrics_eval_device_with_aupro_wall_s": spread(row_aupro),
            "host_over_device_wall": float(np.median(host_s) / np.median(dev_wall))})
        del masks, maps, scores
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print(json.dumps(record))


if __name__ == "__main__":
    main()
