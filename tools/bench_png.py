#!/usr/bin/env python3
"""Time the PNG encoder (csrc/png.hip) on one MI355X against the host encoders, the contenders alternating in one process
and each walking round several copies of its input.

On 64 frames of 1554 x 518 x 3 and 16 frames of 2772 x 924 x 3 (three stacked panels: a photo, the photo under a colour
ramp, the photo with a filled rectangle; the photos are scikit-learn's two sample images where it is installed, else a
seeded blurred random walk), and on 64 one-channel masks of 518 x 518:
(a) pillow   Pillow's PNG writer into memory on 8 threads: the parent commit's encoder
(b) zlib     zlib.compressobj(6, strategy=Z_RLE) over pre-filtered bytes on 8 threads (the filtering is not timed)
(c) device   engine.png_encode, the offsets read, the used payload copied to the host, every stream wrapped into a file
             with its CRC-32 on 8 threads -- everything but the disk write; the wrap is also timed alone
(d) kernels  the two launches alone, with the bytes of input per second
The share of the per-segment code build inside the first launch is not measured: it would need a second build of the
kernel.  File sizes are reported against Pillow's and zlib's.
(f) the overlay pass of a class of 170 images (tools/bench_overlay.py's synthetic tree): eval_overlay.write_overlays, the
    parent commit's pass, against eval_png.write_overlays with encoder="device", alternating.

usage: python tools/bench_png.py [--rounds 3] [--out profiles/png_timing.json] [--no-pass]"""
import argparse
import concurrent.futures
import io
import json
import os
import statistics
import sys
import tempfile
import time
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "aa-clip-iqm_amd"))
import numpy as np
import torch
from PIL import Image

import forward_utils as FU
from aaclip_hip import engine

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "png_timing.json"))
ap.add_argument("--no-pass", action="store_true", help="skip the overlay pass of a class")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_png needs an MI355X; a CPU run measures nothing")
dev = torch.device("cuda:0")
THREADS, COPIES = 8, 2


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}


def photos(side):
    try:
        from sklearn.datasets import load_sample_images
        source = "scikit-learn sample images"
        base = [np.asarray(im) for im in load_sample_images().images]
    except Exception:
        source = "blurred random walk"
        rng = np.random.default_rng(1)
        base = []
        for _ in range(2):
            x = rng.normal(size=(427, 640, 3)).cumsum(0).cumsum(1)
            for axis in (0, 1):
                x = (x + np.roll(x, 1, axis) + np.roll(x, -1, axis)) / 3
            base.append(((x - x.min()) / (x.max() - x.min()) * 255).astype(np.uint8))
    return source, base


def panels(base, n, side, seed):
    """n frames [3 * side, side, 3]: a crop of a photo resized to side x side (bicubic), under a colour ramp, and with a
    filled rectangle"""
    rng = np.random.default_rng(seed)
    ramp = engine.overlay_lut("jet").numpy()[np.linspace(0, 255, side).astype(int)][None].repeat(side, 0).astype(np.int32)
    out = np.empty((n, 3 * side, side, 3), np.uint8)
    for i in range(n):
        src = base[i % len(base)]
        h = int(rng.integers(300, src.shape[0]))
        y, x = int(rng.integers(0, src.shape[0] - h + 1)), int(rng.integers(0, src.shape[1] - h + 1))
        img = np.asarray(Image.fromarray(src[y:y + h, x:x + h]).resize((side, side), Image.BICUBIC)).astype(np.int32)
        boxed = img.copy()
        boxed[side // 4:side // 2, side // 3:side // 3 * 2] = (boxed[side // 4:side // 2, side // 3:side // 3 * 2] + (0, 255, 0)) // 2
        out[i] = np.concatenate([img, (img + ramp + 1) >> 1, boxed]).astype(np.uint8)
    return out


def pillow_bytes(frame):
    buf = io.BytesIO()
    Image.fromarray(frame if frame.ndim == 3 and frame.shape[2] == 3 else frame.reshape(frame.shape[:2])).save(buf, format="PNG")
    return buf.getbuffer().nbytes


def zrle_bytes(filtered):
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    return len(co.compress(filtered) + co.flush())


def gpu_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


source, base = photos(518)
result = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "threads": THREADS, "copies": COPIES,
          "cpus": len(os.sched_getaffinity(0)), "photos": source, "sizes": []}
pool = concurrent.futures.ThreadPoolExecutor(max_workers=THREADS)
for what, n, side, C in (("panels", 64, 518, 3), ("panels", 16, 924, 3), ("masks", 64, 518, 1)):
    if C == 3:
        host = [panels(base, n, side, 7 + k) for k in range(COPIES)]
    else:
        host = []
        for k in range(COPIES):
            m = np.zeros((n, side, side, 1), np.uint8)
            rng = np.random.default_rng(20 + k)
            for i in range(n):
                y, x = rng.integers(0, side // 2, 2)
                m[i, y:y + side // 4, x:x + side // 3] = 255
            host.append(m)
    H, W = host[0].shape[1:3]
    on = [torch.from_numpy(h).to(dev) for h in host]
    filtered = [[FU.png_filter_host(f).tobytes() for f in h] for h in host]
    turn = {"pillow": 0, "zlib": 0, "device": 0, "kernels": 0}
    sizes = {}

    def nxt(key):
        turn[key] = (turn[key] + 1) % COPIES
        return turn[key]

    def run_pillow():
        sizes["pillow"] = list(pool.map(pillow_bytes, host[nxt("pillow")]))

    def run_zlib():
        sizes["zlib"] = list(pool.map(zrle_bytes, filtered[nxt("zlib")]))

    wrap_s = []

    def run_device():
        payload, offsets = engine.png_encode(on[nxt("device")])
        offsets = offsets.cpu().tolist()
        data = payload[:offsets[-1]].cpu().numpy()
        t0 = time.perf_counter()
        files = list(pool.map(lambda i: FU.png_file(data[offsets[i]:offsets[i + 1]], H, W, C), range(n)))
        wrap_s.append(time.perf_counter() - t0)
        sizes["device"] = [len(f) for f in files]
        return files

    files = run_device()                                       # also the warm-up; and the files are what they should be
    for i in (0, n - 1):
        with Image.open(io.BytesIO(files[i])) as im:
            assert np.array_equal(np.array(im).reshape(H, W, C), host[turn["device"]][i]), "a device file decodes to other pixels"
    run_pillow(), run_zlib()
    del wrap_s[:]
    contenders = {"pillow": run_pillow, "zlib": run_zlib, "device": run_device}
    t = {k: [] for k in contenders}
    kernels = []
    for _ in range(a.rounds):                                  # the contenders alternate
        for k, fn in contenders.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            t[k].append((time.perf_counter() - t0) * 1e3)
        kernels.append(gpu_ms(lambda: engine.png_encode(on[nxt("kernels")])))
    med = {k: statistics.median(v) for k, v in t.items()}
    in_bytes = n * H * W * C
    entry = {"what": what, "frames": n, "height": H, "width": W, "channels": C, "input_bytes": in_bytes,
             "ms": {k: spread(v) for k, v in t.items()}, "ms_per_file": {k: v / n for k, v in med.items()},
             "kernels_ms": spread(kernels), "kernels_gbs": in_bytes / (statistics.median(kernels) * 1e-3) / 1e9,
             "wrap_with_crc_ms": spread([s * 1e3 for s in wrap_s]),
             "wrap_share_of_device": statistics.median(wrap_s) * 1e3 / med["device"],
             "pillow_over_device": med["pillow"] / med["device"], "zlib_over_device": med["zlib"] / med["device"],
             "file_bytes": {k: int(sum(v)) for k, v in sizes.items()},
             "device_over_pillow_bytes": sum(sizes["device"]) / sum(sizes["pillow"]),
             "device_over_zlib_bytes": sum(sizes["device"]) / sum(sizes["zlib"])}
    result["sizes"].append(entry)
    print(f"{n} x {H} x {W} x {C}: pillow {med['pillow']:.0f} ms, zlib Z_RLE {med['zlib']:.0f} ms, device end to end "
          f"{med['device']:.1f} ms (wrap + CRC {statistics.median(wrap_s) * 1e3:.1f} ms), the two launches "
          f"{statistics.median(kernels):.2f} ms ({entry['kernels_gbs']:.1f} GB/s of input); file bytes device / pillow "
          f"{entry['device_over_pillow_bytes']:.4f}, device / zlib {entry['device_over_zlib_bytes']:.4f}", flush=True)
    del on

if not a.no_pass:
    import dataset as D
    import eval_overlay as EO
    import eval_png as EP
    N, SRC, S = 170, 900, 518
    gen = torch.Generator(device="cpu").manual_seed(11)
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "MVTec")
        rng = np.random.default_rng(3)
        yy, xx = np.mgrid[0:SRC, 0:SRC]
        for kind, n in (("good", N // 2), ("broken", N - N // 2)):
            os.makedirs(os.path.join(root, "bottle", "test", kind))
            if kind != "good":
                os.makedirs(os.path.join(root, "bottle", "ground_truth", kind))
            for i in range(n):
                shade = 128 + 60 * np.sin(xx / (50.0 + i) + rng.uniform(0, 3)) * np.cos(yy / (70.0 + i))
                img = np.clip(shade[..., None] + rng.integers(-6, 7, (SRC, SRC, 3)), 0, 255).astype(np.uint8)
                Image.fromarray(img).save(os.path.join(root, "bottle", "test", kind, f"{i:03d}.png"), compress_level=1)
                if kind != "good":
                    mask = np.zeros((SRC, SRC), np.uint8)
                    y0, x0 = rng.integers(50, SRC // 2, 2)
                    mask[y0:y0 + 200, x0:x0 + 150] = 255
                    Image.fromarray(mask).save(os.path.join(root, "bottle", "ground_truth", kind, f"{i:03d}_mask.png"))
        meta = os.path.join(tmp, "meta.jsonl")
        D.build_metadata(root, meta)
        ds = D.BaseSingleClassDataset(root, meta, S, "bottle", device_preprocess=True)
        file_names, masks = [], []
        for b in torch.utils.data.DataLoader(ds, batch_size=32, shuffle=False):
            file_names.extend(b["file_name"])
            masks.append((b["mask"] != 0).to(torch.uint8))
        masks = torch.cat(masks).to(dev)
        maps = torch.rand(N, S, S, generator=gen).mul_(0.9).to(dev)
        pred = torch.zeros(N, S, S, dtype=torch.uint8)
        pred[:, 100:220, 150:330] = 1
        pred = pred.to(dev)
        out = os.path.join(tmp, "overlays")
        passes = {"pillow": lambda d: EO.write_overlays(d, ds, masks, maps, file_names, pred, dev),
                  "device": lambda d: EP.write_overlays(d, ds, masks, maps, file_names, pred, dev, encoder="device")}
        EP.write_overlays(os.path.join(out, "warm"), ds, masks, maps, file_names, pred, dev, limit=32, encoder="device")
        t, size = {k: [] for k in passes}, {}
        for r in range(max(1, a.rounds - 1)):
            for k, fn in passes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                paths = fn(os.path.join(out, f"{k}-{r}"))
                t[k].append(time.perf_counter() - t0)
                size[k] = sum(os.path.getsize(p) for p in paths)
        result["pass"] = {"images": N, "source": [SRC, SRC], "side": S, "batch": 32, "writers": EO.OVERLAY_WRITERS,
                          "seconds": {k: spread(v) for k, v in t.items()}, "png_bytes": size,
                          "pillow_over_device": statistics.median(t["pillow"]) / statistics.median(t["device"])}
        print(f"overlay pass of {N} images: eval_overlay.write_overlays {statistics.median(t['pillow']):.2f} s, "
              f"eval_png.write_overlays(encoder='device') {statistics.median(t['device']):.2f} s; bytes {size}", flush=True)

os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(result, f, indent=1)
print("wrote", a.out)
