#!/usr/bin/env python3
"""Time the greedy coreset selection of the support bank (csrc/coreset.hip) on one MI355X against the same greedy loop
written with torch on the device -- per pick torch.mv over fp16 rows, minimum, argmax, nothing read back -- alternating
in one process, and (at the smallest bank) against the numpy definition on this box's CPU.  Beside that, what the
coreset is for: aaclip_support_nearest for 64 images over the coreset bank and over the full bank.

  N in {5 476, 43 808, 286 121} rows (4, 32 and 209 shots of 1369 patches), E = 768, ratios 0.1 and 0.01, selection on rows
  projected to 128 dimensions (dim 128) and on the rows themselves (dim 0).

The rows are random unit rows: the selection's time does not depend on the values (one pass over the rows per pick),
its picks do -- the torch loop's picks are NOT expected to equal the integer selection's (fp16 rounding flips
near-ties), so only the share of equal picks is reported.  Times are wall clock from the call to the end of a device
synchronisation, so the launches of every pick are in them.

usage: python tools/bench_coreset.py [--rounds 3] [--out profiles/coreset_timing.json] [--no-cpu] [--shots 4,32,209]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "aa-clip-iqm_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch

from aaclip_hip import engine

ap = argparse.ArgumentParser()
ap.add_argument("--shots", default="4,32,209")
ap.add_argument("--ratios", default="0.1,0.01")
ap.add_argument("--dims", default="128,0")
ap.add_argument("--images", type=int, default=64)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "coreset_timing.json"))
ap.add_argument("--no-cpu", action="store_true")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_coreset needs an MI355X; a CPU run measures nothing")
dev = torch.device("cuda:0")
P, E = 1369, 768


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def unit_rows(n, width, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, width, generator=g, device=dev), dim=-1)


def torch_greedy(rows16, n):
    """the same greedy loop with torch on the device: fp16 rows, d2 = 2 - 2 cos on unit rows, nothing read back"""
    N = rows16.shape[0]
    min_d = torch.full((N,), float("inf"), dtype=torch.float16, device=dev)
    picks = torch.zeros(n, dtype=torch.int64, device=dev)
    c = torch.zeros(1, dtype=torch.int64, device=dev)
    for t in range(n):
        picks[t:t + 1] = c
        cos = torch.mv(rows16, rows16.index_select(0, c)[0])
        min_d = torch.minimum(min_d, 2.0 - 2.0 * cos)
        c = torch.argmax(min_d).reshape(1)
    return picks


result = {"device": torch.cuda.get_device_name(0), "patches": P, "E": E, "rounds": a.rounds, "selection": [], "search": []}
queries = unit_rows(a.images * P, E, 1)

for K in [int(v) for v in a.shots.split(",")]:
    N = K * P
    full = unit_rows(N, E, 100 + K)
    full_bank = engine.support_bank_rows(full, "fp16")
    for dim in [int(v) for v in a.dims.split(",")]:
        build_ms, rows = wall_ms(lambda: engine.coreset_projected_rows(full, dim, 0) if dim else full)
        quant_ms, (q, norm2) = wall_ms(lambda: engine.coreset_rows(rows))
        rows16 = rows.half()
        width = rows.shape[1]
        for ratio in [float(v) for v in a.ratios.split(",")]:
            n = max(1, math.ceil(ratio * N))
            hip = lambda: engine.coreset_select(q, norm2, n, 0)
            loop = lambda: torch_greedy(rows16, n)
            hip()
            if n <= 1000:
                loop()
            torch.cuda.synchronize()
            t = {"hip": [], "torch": []}
            for r in range(a.rounds):                                   # the contenders alternate
                ms, (picks, radius2, _) = wall_ms(hip)
                t["hip"].append(ms)
                ms, tpicks = wall_ms(loop)
                t["torch"].append(ms)
            same = float((picks.long() == tpicks).float().mean())
            r2 = radius2.cpu().numpy().view(np.uint32)
            med = {k: statistics.median(v) for k, v in t.items()}
            entry = {"shots": K, "bank_rows": N, "dim": dim, "width": width, "ratio": ratio, "picks": n,
                     "int16_row_bytes": 2.0 * N * width, "project_and_normalise_ms": build_ms if dim else 0.0,
                     "quantise_ms": quant_ms, "ms": {k: spread(v) for k, v in t.items()},
                     "us_per_pick": {k: 1e3 * med[k] / n for k in t}, "torch_over_hip": med["torch"] / med["hip"],
                     "hip_row_bytes_per_s": 2.0 * N * width * n / (med["hip"] * 1e-3),
                     "share_of_picks_equal_to_the_torch_loop": same,
                     "covering_radius_cosine_distance": float(r2[-1]) / float(1 << 29)}
            if K == min(int(v) for v in a.shots.split(",")) and not a.no_cpu:
                import coreset_cases as CC
                hq = q.cpu().numpy()
                t0 = time.perf_counter()
                want = CC.definition(hq, n, 0)
                entry["numpy_definition_s"] = time.perf_counter() - t0
                entry["equal_to_the_numpy_definition"] = bool(np.array_equal(want[0], picks.cpu().numpy()) and
                                                              np.array_equal(want[1], r2))
            result["selection"].append(entry)
            print(f"K={K:3d} N={N:6d} dim={dim:3d} ratio={ratio}: {n} picks, hip {med['hip']:.1f} ms ({entry['us_per_pick']['hip']:.1f} us/pick, "
                  f"{entry['hip_row_bytes_per_s'] / 1e12:.2f} TB/s), torch {med['torch']:.1f} ms ({entry['us_per_pick']['torch']:.1f} us/pick), "
                  f"torch/hip {entry['torch_over_hip']:.2f}, equal picks {same:.3f}, radius {entry['covering_radius_cosine_distance']:.4f}"
                  + (f", numpy {entry['numpy_definition_s']:.2f} s equal={entry['equal_to_the_numpy_definition']}" if "numpy_definition_s" in entry else ""),
                  flush=True)
            # what the coreset is for: the search over it against the search over the full bank (fp16 form, 64 images)
            core_bank = engine.support_bank_rows(full.index_select(0, picks.long()), "fp16")
            for fn in (lambda: engine.support_nearest(queries, core_bank), lambda: engine.support_nearest(queries, full_bank)):
                fn()
            s = {"coreset": [], "full": []}
            for r in range(max(a.rounds, 5)):
                s["coreset"].append(wall_ms(lambda: engine.support_nearest(queries, core_bank))[0])
                s["full"].append(wall_ms(lambda: engine.support_nearest(queries, full_bank))[0])
            smed = {k: statistics.median(v) for k, v in s.items()}
            result["search"].append({"shots": K, "bank_rows": N, "dim": dim, "ratio": ratio, "kept_rows": n,
                                     "query_rows": a.images * P, "ms_per_level": {k: spread(v) for k, v in s.items()},
                                     "full_over_coreset": smed["full"] / smed["coreset"]})
            print(f"      search, {a.images} images: coreset bank {smed['coreset']:.3f} ms/level, full bank {smed['full']:.3f} ms/level", flush=True)
            del core_bank
        del rows, rows16, q, norm2
    del full, full_bank

os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(result, f, indent=1)
print("wrote", a.out)
