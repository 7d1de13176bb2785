"""Time of one class's exact F1-max: forward_utils.f1max_eval (a numpy argsort on the host) next to the device path, and
forward_utils.metrics_eval_device with and without the F1-max columns, alternating in one process on the same synthetic
class: N maps of 518 x 518 generated on the device, 3 % positive pixels (tools/bench_metrics.py's class).

  host f1max      wall time of f1max_eval on the normalised host pixels (the sort is the host's own)
  device rows     wall time and device-event time of metrics_eval_device, f1_max False and True alternating; the rows
                  with the columns are compared with metrics_eval(f1_max=True) once per class
  sorts           calls of engine.metrics_sort per row, with and without the columns (the columns must add none)
  entries         device-event time of aaclip_metrics_f1max on the sorted keys and of aaclip_metrics_threshold
                  (normalising on the fly, mask and per-image counts out) on the raw maps

python tools/bench_f1max.py [--images 64 170] [--rounds 2] [--out profiles/f1max_device_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aa-clip-iqm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import forward_utils as FU  # noqa: E402
from aaclip_hip import engine  # noqa: E402
from bench_metrics import S, make_class, timed_device  # noqa: E402


def count_sorts(fn):
    calls, real = [], engine.metrics_sort
    engine.metrics_sort = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        fn()
    finally:
        engine.metrics_sort = real
    return len(calls)


def entry_times(maps, masks):
    """aaclip_metrics_f1max on sorted keys and aaclip_metrics_threshold on the raw maps, device events around each"""
    labels = masks.view(-1)
    rng, _ = engine.metrics_range(maps, labels, S * S)
    norm = engine.metrics_normalise(maps.view(-1), rng)
    keys, labels_sorted, _ = engine.metrics_sort(norm, labels, True)
    del norm
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    engine.metrics_threshold(maps, engine.metrics_f1max(keys, labels_sorted, True), labels=labels, per_image=S * S,
                             range_record=rng)                        # warm-up: code objects, workspace
    torch.cuda.synchronize()
    ev[0].record()
    rec = engine.metrics_f1max(keys, labels_sorted, True)
    ev[1].record()
    torch.cuda.synchronize()
    ev[2].record()
    engine.metrics_threshold(maps, rec, labels=labels, per_image=S * S, range_record=rng)
    ev[3].record()
    torch.cuda.synchronize()
    n = maps.numel()
    thr_s = ev[2].elapsed_time(ev[3]) * 1e-3
    return {"f1max_s": ev[0].elapsed_time(ev[1]) * 1e-3, "threshold_s": thr_s,
            "threshold_bytes": 6 * n, "threshold_bytes_per_s": 6 * n / thr_s}      # 4 + 1 in, 1 out per element


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[64, 170])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f1max_device_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("tools/bench_f1max.py measures on an MI355X; there is no CPU fallback")
    dev = torch.device("cuda:0")
    record = {"device": torch.cuda.get_device_name(0), "map_size": S, "positive_pixel_share": 0.03, "rounds": args.rounds,
              "classes": []}
    for n_img in args.images:
        masks, labels, maps, scores = make_class(n_img, dev, seed=n_img)
        row = lambda f1: FU.metrics_eval_device(masks, labels, maps, scores, f"n{n_img}", "Industrial", f1_max=f1)  # noqa: E731
        row(True), row(False)                                                    # warm-up: sizes the workspace
        sorts = {"without": count_sorts(lambda: row(False)), "with": count_sorts(lambda: row(True))}
        h_masks, h_maps, h_scores = masks.float().cpu().numpy(), maps.cpu().numpy(), scores.cpu().numpy()
        row_host = FU.metrics_eval(h_masks, labels, h_maps, h_scores, f"n{n_img}", "Industrial", f1_max=True)
        h_norm = (h_maps - h_maps.min()) / (h_maps.max() - h_maps.min())
        host_s, wall, event, entries = [], {False: [], True: []}, {False: [], True: []}, []
        rows_equal = True
        for r in range(args.rounds):
            t0 = time.perf_counter()
            host_f1 = FU.f1max_eval(h_masks, h_norm)
            host_s.append(time.perf_counter() - t0)
            for _ in range(3):
                for f1 in (False, True):
                    got, w, e = timed_device(lambda: row(f1))
                    wall[f1].append(w)
                    event[f1].append(e)
                    rows_equal = rows_equal and (got == row_host if f1 else got == {k: v for k, v in row_host.items() if "F1" not in k})
            entries.append(entry_times(maps, masks))
            print(f"N={n_img} round {r}: host f1max_eval {host_s[-1]:.2f} s; device rows without {wall[False][-3:]} s, with "
                  f"{wall[True][-3:]} s; sorts {sorts}; rows equal: {rows_equal}; {entries[-1]}", flush=True)
        _, dev_f1 = engine.f1max_metrics(maps, masks, per_image=S * S)
        record["classes"].append({
            "images": n_img, "pixels": n_img * S * S, "tie_groups": dev_f1.groups, "f1max": dev_f1._asdict(),
            "f1max_equals_host": dev_f1 == host_f1, "row": got, "rows_equal_host": rows_equal, "sorts_per_row": sorts,
            "host_f1max_eval_wall_s": host_s,
            "device_row_wall_s": {"without": wall[False], "with": wall[True]},
            "device_row_event_s": {"without": event[False], "with": event[True]},
            "columns_cost_wall_s": float(np.median(wall[True]) - np.median(wall[False])),
            "device_entries_event_s": entries})
        del masks, maps, scores, h_masks, h_maps, h_norm
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print(json.dumps(record))


if __name__ == "__main__":
    main()
