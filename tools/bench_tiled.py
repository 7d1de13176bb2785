#!/usr/bin/env python3
"""Time tiled inference (csrc/tiles.hip) on one MI355X against what a user would write in torch instead, alternating in
one process:

  gather   engine.tile_gather of normalised frames [frames, 3, C, C]      vs  slicing + torch.stack
  stitch   engine.tile_stitch of tile maps [frames * G^2, 518, 518]       vs  a weighted accumulate per tile + one divide
           (the torch form blends every pixel, so a pixel under one tile is w * v / w, not that tile's bits)

at (16 frames, G = 2, O = 112: C = 924) and (7 frames, G = 3, O = 112: C = 1330), S = 518; every contender walks round six
copies of its input, more than the Infinity Cache holds.  Reports per case the time per
call (median, min, max over the rounds) and the achieved GB/s over the bytes the operation must move (gather: canvas bytes
read once + tile bytes written; stitch: tile bytes read + canvas bytes written) beside the 6.29 TB/s copy rate the README
quotes.  Then one eval_tiled.get_predictions_tiled batch of 16 frames at G = 2 (64 tiles) against the same 64 model inputs
untiled (eval_last.get_predictions, no gather, no stitch): as G^2 = 4 batches of 16 and as one batch of 64, on the synthetic
ViT-L/14 of bench.py.

usage: python tools/bench_tiled.py [--rounds 7] [--repeats 300] [--out profiles/tiled_timing.json] [--no-model]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "aa-clip-iqm_amd"))
import torch

from aaclip_hip import engine

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--repeats", type=int, default=300, help="calls per timed window")
ap.add_argument("--precision", default="fp16x2")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tiled_timing.json"))
ap.add_argument("--no-model", action="store_true", help="skip the end-to-end batch")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_tiled needs an MI355X; a CPU run measures nothing")
dev = torch.device("cuda:0")
S, O = 518, 112
COPY_RATE_GBS = 6290.0        # README: the copy rate measured on this part
COPIES = 6                    # input copies per contender: 6 x 68 MB of tile maps, the smallest input, pass 256 MiB


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


def origins(G):
    T = S - O
    return [(i * T, j * T) for i in range(G) for j in range(G)]


result = {"device": torch.cuda.get_device_name(0), "tile": S, "overlap": O, "rounds": a.rounds, "repeats": a.repeats,
          "copy_rate_gbs": COPY_RATE_GBS, "cases": []}
gen = torch.Generator(device="cpu").manual_seed(5)
for frames, G in ((16, 2), (7, 3)):
    C = engine.tile_canvas(S, G, O)
    org = origins(G)
    # every contender walks round COPIES copies of its input, more bytes than the 256 MiB Infinity Cache holds, so a
    # call reads what an earlier call of the window has not left there
    canvases = [torch.randn(frames, 3, C, C, generator=gen).to(dev) for _ in range(COPIES)]
    maps = [torch.randn(frames * G * G, S, S, generator=gen).to(dev) for _ in range(COPIES)]
    turn = {"gather_hip": 0, "gather_torch": 0, "stitch_hip": 0, "stitch_torch": 0}
    w1 = torch.minimum(torch.arange(S) + 1, S - torch.arange(S)).float().to(dev)
    w = w1[:, None] * w1[None, :]
    den = torch.zeros(C, C, device=dev)
    for r, c in org:
        den[r:r + S, c:c + S] += w

    def pick(which, copies):
        turn[which] = (turn[which] + 1) % COPIES
        return copies[turn[which]]

    def gather_hip(canvas=None):
        return engine.tile_gather(pick("gather_hip", canvases) if canvas is None else canvas, S, G, O)

    def gather_torch(canvas=None):
        canvas = pick("gather_torch", canvases) if canvas is None else canvas
        return torch.stack([canvas[:, :, r:r + S, c:c + S] for r, c in org], dim=1).reshape(frames * G * G, 3, S, S)

    def stitch_hip(tile_maps=None):
        return engine.tile_stitch(pick("stitch_hip", maps) if tile_maps is None else tile_maps, G, O, frames)

    def stitch_torch(tile_maps=None):
        v = (pick("stitch_torch", maps) if tile_maps is None else tile_maps).view(frames, G * G, S, S)
        out = torch.zeros(frames, C, C, device=dev)
        for t, (r, c) in enumerate(org):
            out[:, r:r + S, c:c + S] += w * v[:, t]
        return out.div_(den)

    same_gather = bool(torch.equal(gather_hip(canvases[0]), gather_torch(canvases[0])))
    stitch_diff = float((stitch_hip(maps[0]) - stitch_torch(maps[0])).abs().max())
    contenders = {"gather_hip": gather_hip, "gather_torch": gather_torch, "stitch_hip": stitch_hip, "stitch_torch": stitch_torch}
    for fn in contenders.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in contenders}
    for _ in range(a.rounds):                          # the contenders alternate
        for k, fn in contenders.items():
            t[k].append(timed(fn, a.repeats))
    need = {"gather": 4.0 * frames * 3 * C * C + 4.0 * frames * G * G * 3 * S * S,
            "stitch": 4.0 * frames * G * G * S * S + 4.0 * frames * C * C}
    med = {k: statistics.median(v) for k, v in t.items()}
    gbs = {k: need[k.split("_")[0]] / (med[k] * 1e-3) / 1e9 for k in t}
    entry = {"frames": frames, "grid": G, "canvas": C, "tiles": frames * G * G, "bytes_needed": need,
             "gather_equal_to_torch": same_gather, "stitch_max_abs_difference_to_torch": stitch_diff,
             "ms": {k: spread(v) for k, v in t.items()}, "gbs": gbs,
             "share_of_copy_rate": {k: v / COPY_RATE_GBS for k, v in gbs.items()},
             "torch_over_hip": {"gather": med["gather_torch"] / med["gather_hip"],
                                "stitch": med["stitch_torch"] / med["stitch_hip"]}}
    result["cases"].append(entry)
    print(f"{frames} frames, G = {G} (C = {C}): gather hip {med['gather_hip']:.3f} ms ({gbs['gather_hip']:.0f} GB/s), torch "
          f"{med['gather_torch']:.3f} ms ({gbs['gather_torch']:.0f} GB/s); stitch hip {med['stitch_hip']:.3f} ms "
          f"({gbs['stitch_hip']:.0f} GB/s), torch {med['stitch_torch']:.3f} ms ({gbs['stitch_torch']:.0f} GB/s)", flush=True)
    del canvases, maps

if not a.no_model:
    import eval_last as EL
    import eval_tiled as ET
    from aaclip_hip import synth
    from model.adapter import AdaptedCLIP
    from model.clip import create_model
    cfg = synth.ClipCfg()
    clip = create_model("ViT-L-14-336", S, pretrained=None, precision=a.precision, force_image_size=S)
    clip.load_state_dict(synth.synth_clip_state_dict(cfg, 111), strict=True)
    model = AdaptedCLIP(clip, relu=False)
    model.image_adapter.load_state_dict(synth.synth_image_adapter_state_dict(cfg, seed=111), strict=True)
    model.text_adapter.load_state_dict(synth.synth_text_adapter_state_dict(cfg, seed=111), strict=True)
    model = model.to(dev).eval()
    anchors = torch.nn.functional.normalize(torch.randn(768, 2, generator=gen), dim=0).to(dev)
    frames, G = 16, 2
    C = engine.tile_canvas(S, G, O)

    def batch(n, side):
        return {"image": torch.randn(n, 3, side, side, generator=gen).to(dev), "mask": torch.zeros(n, 1, side, side),
                "label": torch.zeros(n, dtype=torch.int64), "file_name": ["f"] * n, "class_name": ["c"] * n}

    loaders = {"tiled": [batch(frames, C)], "untiled_batches": [batch(frames, S) for _ in range(G * G)],
               "untiled_one_batch": [batch(frames * G * G, S)]}

    def tiled():
        with torch.no_grad():
            return ET.get_predictions_tiled(model, anchors, loaders["tiled"], dev, S, "MVTec", use_iqm=False, on_device=True,
                                            tiles=(G, O))

    def untiled(which):
        with torch.no_grad():
            return EL.get_predictions(model, anchors, loaders[which], dev, S, "MVTec", use_iqm=False, on_device=True)

    contenders = {"tiled": tiled, "untiled_batches": lambda: untiled("untiled_batches"),
                  "untiled_one_batch": lambda: untiled("untiled_one_batch")}
    for fn in contenders.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in contenders}
    for _ in range(a.rounds):
        for k, fn in contenders.items():
            t[k].append(timed(fn, 1))
    med = {k: statistics.median(v) for k, v in t.items()}
    result["batch"] = {"precision": a.precision, "frames": frames, "grid": G, "canvas": C, "model_inputs": frames * G * G,
                       "ms": {k: spread(v) for k, v in t.items()},
                       "tiled_over_untiled_batches": med["tiled"] / med["untiled_batches"],
                       "tiled_over_untiled_one_batch": med["tiled"] / med["untiled_one_batch"],
                       "added_ms_over_one_batch": med["tiled"] - med["untiled_one_batch"]}
    print(f"one tiled batch ({frames} frames, {frames * G * G} tiles): {med['tiled']:.1f} ms; the same inputs untiled as "
          f"{G * G} batches of {frames}: {med['untiled_batches']:.1f} ms, as one batch: {med['untiled_one_batch']:.1f} ms",
          flush=True)

os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(result, f, indent=1)
print("wrote", a.out)
