#!/usr/bin/env python3
"""Time the heat-map overlays (csrc/overlay.hip) on one MI355X, the contenders alternating in one process.

(a) the kernel: engine.overlay_render at 64 frames of 518 x 518 and 16 frames of 924 x 924, three panels, both masks,
    T = 1 and T = 3, against the same bytes written in torch (table lookup, integer blend, max_pool2d for the contour;
    the number of bytes in which it differs is recorded: torch divides by a scalar through its reciprocal) and against
    the numpy definition on the host (forward_utils.render_overlays_host, on --host-frames frames, reported per frame).  Every device contender walks round two copies of its input (each copy is
    larger than the 256 MiB Infinity Cache).  Reported as ms per call and as TB/s over the bytes the operation must move
    -- 12 of frame, 4 of map, 2 of masks read and 9 of panels written per pixel, 27 -- beside the 6.29 TB/s copy rate.
(b) the overlay pass of a class of 170 images (synthetic 900 x 900 PNGs with 85 masks, written to a temporary tree and
    read through dataset.BaseSingleClassDataset with device_preprocess, maps of 518 x 518): eval_overlay.write_overlays as
    a whole, and its steps one after the other -- decode (the loader's second walk), render (upload, engine.preprocess,
    engine.overlay_render), copy (panels to the host) and encode (Pillow's PNG writer on 8 threads).

usage: python tools/bench_overlay.py [--rounds 5] [--repeats 20] [--out profiles/overlay_timing.json] [--no-pass]"""
import argparse
import concurrent.futures
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "aa-clip-iqm_amd"))
import numpy as np
import torch

from aaclip_hip import engine

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--repeats", type=int, default=20, help="calls per timed window")
ap.add_argument("--host-frames", type=int, default=4, help="frames of the numpy definition's run")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "overlay_timing.json"))
ap.add_argument("--no-pass", action="store_true", help="skip the overlay pass of a class")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_overlay needs an MI355X; a CPU run measures nothing")
dev = torch.device("cuda:0")
COPY_RATE_GBS = 6290.0        # README: the copy rate measured on this part
BYTES_PER_PIXEL = 12 + 4 + 2 + 9
COPIES = 2
ALPHA256 = 128
MEAN = torch.tensor(engine.CLIP_MEAN, device=dev).view(1, 3, 1, 1)
STD = torch.tensor(engine.CLIP_STD, device=dev).view(1, 3, 1, 1)
PRED_COLOUR = torch.tensor([255, 255, 255], dtype=torch.int32, device=dev)
TRUTH_COLOUR = torch.tensor([0, 255, 0], dtype=torch.int32, device=dev)
LUT = engine.overlay_lut("jet").to(dev)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}


def timed(fn, repeats):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(repeats):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / repeats


def blobs(gen, B, H, W):
    """uint8 masks: three rectangles per image, about a tenth of the pixels"""
    m = torch.zeros(B, H, W, dtype=torch.uint8)
    for b in range(B):
        for _ in range(3):
            h, w = (int(torch.randint(H // 16, H // 4, (1,), generator=gen)) for _ in range(2))
            y, x = int(torch.randint(0, H - h, (1,), generator=gen)), int(torch.randint(0, W - w, (1,), generator=gen))
            m[b, y:y + h, x:x + w] = 1
    return m


def contour_torch(mask, T):
    m = mask != 0
    near = torch.nn.functional.max_pool2d((~m).float().unsqueeze(1), 2 * T + 1, stride=1, padding=T).squeeze(1) > 0
    return m & near                  # the pooling pads with -inf: pixels outside the image count as nothing


def render_torch(frames, maps, mn, mx, pred, truth, T):
    """the bytes of engine.overlay_render(frames, maps, record, pred, truth, alpha=0.5, thickness=T) in torch"""
    v = torch.round(((frames * STD) + MEAN) * 255)
    F = torch.nan_to_num(v, nan=0.0, posinf=255.0, neginf=0.0).clamp_(0, 255).to(torch.int32).permute(0, 2, 3, 1)
    n = (maps - mn) / float(np.float32(mx) - np.float32(mn)) if mx != 1.0 else maps       # the span is an fp32 subtraction
    q = torch.where(torch.isnan(n), torch.zeros_like(n), n.clamp(0, 1)).double().mul_(255.0).floor_().long()
    heat = (ALPHA256 * F + (256 - ALPHA256) * LUT[q].to(torch.int32) + 128) >> 8
    filled = (ALPHA256 * F + (256 - ALPHA256) * TRUTH_COLOUR + 128) >> 8
    panel = torch.where((truth != 0).unsqueeze(-1), filled, F)
    panel[contour_torch(truth, T)] = TRUTH_COLOUR
    cp = contour_torch(pred, T)
    heat[cp] = PRED_COLOUR
    panel[cp] = PRED_COLOUR
    return torch.cat([F, heat, panel], dim=1).to(torch.uint8)


result = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "repeats": a.repeats, "copy_rate_gbs": COPY_RATE_GBS,
          "bytes_per_pixel": BYTES_PER_PIXEL, "alpha256": ALPHA256, "kernel": []}
gen = torch.Generator(device="cpu").manual_seed(11)
for B, side in ((64, 518), (16, 924)):
    inputs = []
    for _ in range(COPIES):
        frames = torch.randn(B, 3, side, side, generator=gen).to(dev)
        maps = torch.rand(B, side, side, generator=gen).mul_(0.9).to(dev)
        inputs.append((frames, maps, engine.metrics_range(maps)[0], blobs(gen, B, side, side).to(dev),
                       blobs(gen, B, side, side).to(dev)))
    ranges = [engine.metrics_range_host(i[2]) for i in inputs]
    for T in (1, 3):
        turn = {"hip": 0, "torch": 0}

        def hip(k=None):
            turn["hip"] = (turn["hip"] + 1) % COPIES
            f, m, r, p, g = inputs[turn["hip"] if k is None else k]
            return engine.overlay_render(f, m, r, p, g, alpha=0.5, thickness=T)

        def in_torch(k=None):
            turn["torch"] = (turn["torch"] + 1) % COPIES
            k = turn["torch"] if k is None else k
            f, m, r, p, g = inputs[k]
            return render_torch(f, m, ranges[k]["min"], ranges[k]["max"], p, g, T)

        differing = int((hip(0) != in_torch(0)).sum())
        equal = differing == 0
        contenders = {"hip": hip, "torch": in_torch}
        for fn in contenders.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in contenders}
        for _ in range(a.rounds):                          # the contenders alternate
            for k, fn in contenders.items():
                t[k].append(timed(fn, a.repeats if k == "hip" else max(2, a.repeats // 5)))
        n_host = min(a.host_frames, B)
        f, m, r, p, g = (x[:n_host].cpu() if x.dim() > 1 else x.cpu() for x in inputs[0])
        import forward_utils as FU
        t0 = time.perf_counter()
        host = FU.render_overlays_host(f, m, r, p, g, alpha256=ALPHA256, thickness=T)
        host_ms = (time.perf_counter() - t0) * 1e3
        host_equal = bool(np.array_equal(host, hip(0)[:n_host].cpu().numpy()))
        need = float(BYTES_PER_PIXEL) * B * side * side
        med = {k: statistics.median(v) for k, v in t.items()}
        tbs = {k: need / (med[k] * 1e-3) / 1e12 for k in t}
        result["kernel"].append({
            "frames": B, "side": side, "thickness": T, "bytes_needed": need, "equal_to_torch": equal,
            "bytes_differing_from_torch": differing,
            "equal_to_numpy": host_equal, "ms": {k: spread(v) for k, v in t.items()}, "tbs": tbs,
            "share_of_copy_rate": {k: v * 1e3 / COPY_RATE_GBS for k, v in tbs.items()},
            "torch_over_hip": med["torch"] / med["hip"],
            "numpy": {"frames": n_host, "ms": host_ms, "ms_per_frame": host_ms / n_host,
                      "ms_for_all_frames_extrapolated": host_ms / n_host * B}})
        print(f"{B} x {side}^2, T = {T}: hip {med['hip']:.3f} ms ({tbs['hip']:.2f} TB/s, "
              f"{100 * tbs['hip'] * 1e3 / COPY_RATE_GBS:.0f} % of the copy rate), torch {med['torch']:.2f} ms "
              f"({tbs['torch']:.3f} TB/s), numpy {host_ms / n_host:.0f} ms per frame; equal: torch {equal}, numpy {host_equal}",
              flush=True)
    del inputs

if not a.no_pass:
    import dataset as D
    import eval_overlay as EO
    from PIL import Image
    N, SRC, S = 170, 900, 518
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "MVTec")
        rng = np.random.default_rng(3)
        yy, xx = np.mgrid[0:SRC, 0:SRC]
        for kind, n in (("good", N // 2), ("broken", N - N // 2)):
            os.makedirs(os.path.join(root, "bottle", "test", kind))
            if kind != "good":
                os.makedirs(os.path.join(root, "bottle", "ground_truth", kind))
            for i in range(n):
                base = 128 + 60 * np.sin(xx / (50.0 + i) + rng.uniform(0, 3)) * np.cos(yy / (70.0 + i))
                img = np.clip(base[..., None] + rng.integers(-6, 7, (SRC, SRC, 3)), 0, 255).astype(np.uint8)
                Image.fromarray(img).save(os.path.join(root, "bottle", "test", kind, f"{i:03d}.png"))
                if kind != "good":
                    mask = np.zeros((SRC, SRC), np.uint8)
                    y0, x0 = rng.integers(50, SRC // 2, 2)
                    mask[y0:y0 + 200, x0:x0 + 150] = 255
                    Image.fromarray(mask).save(os.path.join(root, "bottle", "ground_truth", kind, f"{i:03d}_mask.png"))
        meta = os.path.join(tmp, "meta.jsonl")
        D.build_metadata(root, meta)
        ds = D.BaseSingleClassDataset(root, meta, S, "bottle", device_preprocess=True)
        assert len(ds) == N
        loader = lambda: torch.utils.data.DataLoader(ds, batch_size=32, shuffle=False)
        file_names, masks = [], []
        for b in loader():
            file_names.extend(b["file_name"])
            masks.append((b["mask"] != 0).to(torch.uint8))
        masks = torch.cat(masks).to(dev)
        maps = torch.rand(N, S, S, generator=gen).mul_(0.9).to(dev)
        pred = blobs(gen, N, S, S).to(dev)
        out = os.path.join(tmp, "overlays")
        EO.write_overlays(os.path.join(out, "warm"), ds, masks, maps, file_names, pred, dev, limit=32)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        paths = EO.write_overlays(os.path.join(out, "whole"), ds, masks, maps, file_names, pred, dev)
        whole = time.perf_counter() - t0
        png_bytes = sum(os.path.getsize(p) for p in paths)
        # the steps one after the other
        steps = {"decode": 0.0, "render": 0.0, "copy": 0.0, "encode": 0.0}
        record = engine.metrics_range(maps)[0]
        os.makedirs(os.path.join(out, "steps"))
        done = 0
        with concurrent.futures.ThreadPoolExecutor(max_workers=EO.OVERLAY_WRITERS) as pool:
            it = iter(loader())
            while True:
                t0 = time.perf_counter()
                batch = next(it, None)
                steps["decode"] += time.perf_counter() - t0
                if batch is None:
                    break
                b = len(batch["file_name"])
                t0 = time.perf_counter()
                image = engine.preprocess(batch["image"].to(dev), S)
                panels = engine.overlay_render(image, maps[done:done + b].contiguous(), record, pred[done:done + b].contiguous(),
                                               masks[done:done + b].reshape(b, S, S).contiguous(), alpha=0.5, thickness=1)
                torch.cuda.synchronize()
                steps["render"] += time.perf_counter() - t0
                t0 = time.perf_counter()
                host = panels.cpu().numpy()
                steps["copy"] += time.perf_counter() - t0
                t0 = time.perf_counter()
                for f in [pool.submit(EO._save_png, os.path.join(out, "steps", f"{done + i}.png"), host[i]) for i in range(b)]:
                    f.result()
                steps["encode"] += time.perf_counter() - t0
                done += b
        total = sum(steps.values())
        result["pass"] = {"images": N, "source": [SRC, SRC], "side": S, "batch": 32, "writers": EO.OVERLAY_WRITERS,
                          "cpus": len(os.sched_getaffinity(0)), "whole_s": whole, "steps_s": steps, "steps_total_s": total,
                          "share": {k: v / total for k, v in steps.items()}, "png_bytes": png_bytes,
                          "panel_bytes": N * 3 * S * S * 3}
        print(f"overlay pass of {N} images: {whole:.2f} s as a whole; decode {steps['decode']:.2f} s, render "
              f"{steps['render']:.3f} s, copy {steps['copy']:.3f} s, encode {steps['encode']:.2f} s", flush=True)

os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(result, f, indent=1)
print("wrote", a.out)
