#!/usr/bin/env python3
"""Time AdaptedCLIP.encode_text forward + backward (HIP kernels, aaclip_hip.autograd.TextTower) on the full-size text
tower (768 / 12 heads / 12 layers, text_adapt_until = 3, synthetic weights) at 16 and 256 sentences, against torch
autograd of the oracle's adapted_encode_text in fp32 on the same GPU.  The two are run alternately in one process; the
medians, minima and spreads of both go into one JSON line (and --out FILE).

    python tools/bench_text_train.py --rounds 7 --out text_train_bench.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_text_train.py --rounds 2 --only-hip --sentences 256
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "aa-clip-iqm_amd"), REPO):
    sys.path.insert(0, p)

from aaclip_hip import synth  # noqa: E402
import oracle.aaclip_oracle as O  # noqa: E402


def build(dev, precision):
    from model.adapter import AdaptedCLIP
    from model.model import CLIP
    cfg = synth.ClipCfg(image_size=70, vision=synth.TowerCfg(256, 1, 4, 1024))     # the image side is not used
    sd = synth.synth_clip_state_dict(cfg, seed=111)
    ta = synth.synth_text_adapter_state_dict(cfg, until=3, seed=111)
    clip = CLIP(cfg.embed_dim, dict(image_size=70, layers=1, width=256, patch_size=14),
                dict(context_length=77, vocab_size=cfg.vocab_size, width=768, heads=12, layers=12), precision=precision)
    clip.load_state_dict(sd, strict=True)
    model = AdaptedCLIP(clip, text_adapt_until=3, image_adapt_until=1, levels=[1], relu=False)
    model.text_adapter.load_state_dict(ta, strict=True)
    for p in model.parameters():
        p.requires_grad_(False)
    for p in model.text_adapter.parameters():
        p.requires_grad_(True)
    return cfg, sd, ta, model.to(dev).eval()


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sentences", type=int, nargs="*", default=[16, 256])
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--only-hip", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg, sd, ta, model = build(dev, args.precision)
    sd_dev = {k: v.to(dev) for k, v in sd.items() if not k.startswith("visual.")}
    ta_dev = {k: v.to(dev).requires_grad_(True) for k, v in ta.items()}
    result = {"tool": "bench_text_train", "precision": args.precision, "rounds": args.rounds, "cases": {}}
    for n in args.sentences:
        g = torch.Generator().manual_seed(n)
        tok = torch.randint(1, 49000, (n, 77), generator=g, dtype=torch.int32)
        for i in range(n):
            e = 4 + (i * 7) % 70
            tok[i, e] = 49407
            tok[i, e + 1:] = 0
        tok_dev = tok.to(dev)
        d_out = torch.randn(n, cfg.embed_dim, generator=g).to(dev)

        def hip():
            model.zero_grad(set_to_none=True)
            model.encode_text(tok_dev).backward(d_out)

        def ref():
            for v in ta_dev.values():
                v.grad = None
            O.adapted_encode_text(tok_dev, sd_dev, ta_dev, 12, text_adapt_until=3).backward(d_out)

        arms = {"hip": hip} if args.only_hip else {"hip": hip, "torch_autograd_fp32": ref}
        times = {k: [] for k in arms}
        for fn in arms.values():            # warm-up: workspaces, weight caches, torch's kernel selection
            fn()
            fn()
        for _ in range(args.rounds):        # alternate the arms inside one process
            for k, fn in arms.items():
                times[k].append(timed(fn, dev))
        case = {}
        for k, v in times.items():
            case[k] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
                       "spread_pct": 100.0 * (max(v) - min(v)) / statistics.median(v), "samples_ms": v}
        if not args.only_hip:
            case["hip_over_torch"] = case["hip"]["median_ms"] / case["torch_autograd_fp32"]["median_ms"]
        result["cases"][f"sentences_{n}"] = case
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
