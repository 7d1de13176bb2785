"""Time of one class's defect instances at an operating point: forward_utils.defects_eval (numpy + scipy.ndimage on the
host) next to forward_utils.defects_eval_device (csrc/region_table.hip), alternating in one process on the same
synthetic class: N maps of 518 x 518 generated on the device, ground truth from smooth random fields (the "blobs" of
tests/pro_cases.py).  The two results are compared too.

  host      wall time of defects_eval on host arrays (the copy of maps and masks to the host is timed on its own)
  device    wall time and device-event time of defects_eval_device on the device tensors, lists on the host
  table     device-event time of aaclip_region_table alone (engine.region_table on a labelled mask, repeated), next to
            the aaclip_metrics_regions call in front of it and to the bytes the table pass reads (region + area + scores
            + other = 13 B per pixel): the rate and its share of the measured float4 copy rate of the part, 6.29 TB/s
  full      the same for the "full" pattern -- one region per image, every pixel of a workgroup on one row: the
            contention worst case

python tools/bench_defects.py [--images 64 170] [--rounds 3] [--out profiles/defects_device_timing.json]"""
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
MIN_AREA = 9
BYTES_PER_PIXEL = 13
COPY_RATE = 6.29e12             # measured float4 copy on the part (8 TB/s on paper)
TABLE_REPEATS = 20


def make_class(n_img, dev, seed):
    """masks: a smooth random field above its 0.9 quantile (a handful of blobs per image); maps: noise + the mask"""
    g = torch.Generator(device=dev).manual_seed(seed)
    field = torch.randn(n_img, 1, S // 14, S // 14, device=dev, generator=g)
    field = torch.nn.functional.interpolate(field, size=(S, S), mode="bicubic", align_corners=False)[:, 0]
    masks = (field > torch.quantile(field.flatten()[::97], 0.9)).to(torch.uint8).contiguous()
    maps = (torch.randn(n_img, S, S, device=dev, generator=g) * 0.3 + 1.5 * masks.float()).contiguous()
    return masks, maps


def timed_device(fn, repeats=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(repeats):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) / repeats, a.elapsed_time(b) * 1e-3 / repeats


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "all": [float(x) for x in v]}


def table_alone(mask, maps, other, rng, rounds):
    """-> event times of metrics_regions and of region_table alone on its outputs, the latter over TABLE_REPEATS calls"""
    regions_s, table_s = [], []
    for _ in range(rounds):
        (region, area, record), _, ev = timed_device(lambda: engine.metrics_regions(mask))
        regions_s.append(ev)
        count = int(record.cpu()[0])
        engine.region_table(region, area, maps, other=other, range_record=rng, min_area=MIN_AREA, kept_mask=True, regions=count)
        _, _, ev = timed_device(lambda: engine.region_table(region, area, maps, other=other, range_record=rng,
                                                            min_area=MIN_AREA, kept_mask=True, regions=count), TABLE_REPEATS)
        table_s.append(ev)
    rate = mask.numel() * BYTES_PER_PIXEL / float(np.median(table_s))
    return {"regions": count, "metrics_regions_event_s": spread(regions_s), "region_table_event_s": spread(table_s),
            "region_table_read_bytes": mask.numel() * BYTES_PER_PIXEL, "region_table_bytes_per_s": rate,
            "share_of_copy_rate": rate / COPY_RATE,
            "table_over_regions": float(np.median(table_s) / np.median(regions_s))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[64, 170])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "defects_device_timing.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    record = {"device": torch.cuda.get_device_name(0), "map_size": S, "min_area": MIN_AREA, "rounds": args.rounds,
              "table_repeats": TABLE_REPEATS, "copy_rate_bytes_per_s": COPY_RATE, "classes": []}
    for n_img in args.images:
        masks, maps = make_class(n_img, dev, seed=n_img)
        records = {}
        _, f1 = engine.f1max_metrics(maps, masks, per_image=S * S, records=records)
        rng, f1_record = records["range"], records["f1max"]
        FU.defects_eval_device(masks, maps, f1_record, MIN_AREA, range_record=rng)          # warm-up: sizes the workspace
        host_s, d2h_s, dev_wall, dev_event, equal = [], [], [], [], []
        for r in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h_masks, h_maps = masks.cpu().numpy(), engine.metrics_normalise(maps, rng).cpu().numpy()
            d2h_s.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            host = FU.defects_eval(h_masks, h_maps, f1.threshold, MIN_AREA)
            host_s.append(time.perf_counter() - t0)
            del h_masks, h_maps
            for _ in range(3):
                got, wall, event = timed_device(lambda: FU.defects_eval_device(masks, maps, f1_record, MIN_AREA, range_record=rng))
                dev_wall.append(wall)
                dev_event.append(event)
                equal.append(all(got[k] == host[k] for k in FU.DEFECT_COLS + ["record", "predicted", "truth"]))
            print(f"N={n_img} round {r}: host {host_s[-1]:.2f} s (+ {d2h_s[-1]:.2f} s copy), device wall {dev_wall[-3:]} s, "
                  f"events {dev_event[-3:]} s, equal {equal[-3:]}", flush=True)
        predicted = engine.metrics_threshold(maps, f1_record, range_record=rng, totals=False)[0]
        blobs = table_alone(predicted, maps, masks, rng, args.rounds)
        full = table_alone(torch.ones_like(masks), maps, masks, rng, args.rounds)
        print(f"N={n_img}: table alone {blobs}; full {full}", flush=True)
        record["classes"].append({
            "images": n_img, "pixels": n_img * S * S, "threshold": f1.threshold, "record": list(host["record"]),
            "columns": {k: host[k] for k in FU.DEFECT_COLS}, "device_equals_host": bool(all(equal)),
            "host_defects_eval_wall_s": spread(host_s), "host_copy_wall_s": spread(d2h_s),
            "device_defects_eval_wall_s": spread(dev_wall), "device_defects_eval_event_s": spread(dev_event),
            "host_over_device_wall": float(np.median(host_s) / np.median(dev_wall)),
            "table_at_the_operating_point": blobs, "table_full_pattern": full})
        del masks, maps, predicted
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print(json.dumps(record))


if __name__ == "__main__":
    main()
