"""engine.block_backward of one visual-tower block (L = 1370, D = 1024, 16 heads, F = 4096) in both backward
arithmetics, fp32 and bf16x3, in ONE process ("The bf16x3 backward").

Default: HIP-event timings.  For every (batch, adapter) it warms both modes up, then alternates fp32 / bf16x3 calls,
`--calls` each, every call between its own pair of events; the attention backward alone is timed the same way.  One JSON
line on stdout, the same object in --out.  The baseline is always the fp32 entry timed in this very run.

--trace: no timing, `--calls` calls per mode at the first batch with an adapter, for a
`rocprofv3 --kernel-trace --stats -- python tools/time_block_backward_bf16x3.py --trace` run (tracing only); the kernel
names tell the modes apart (attn_bwd_* against attn3_*, gemm32_kernel against gemm16_kernel / the 256-tile kernels,
split3_kernel)."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "aa-clip-iqm_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from aaclip_hip import engine, synth  # noqa: E402
from model.model import CLIP  # noqa: E402

MODES = ("fp32", "bf16x3")
D, H, F = 1024, 16, 4096


def build_block(dev):
    cfg = synth.ClipCfg(embed_dim=256, image_size=70, vision=synth.TowerCfg(D, 1, H, F), text=synth.TowerCfg(256, 1, 4, 1024))
    clip = CLIP(cfg.embed_dim, dict(image_size=70, layers=1, width=D, patch_size=14),
                dict(context_length=77, vocab_size=cfg.vocab_size, width=256, heads=4, layers=1), precision="fp32")
    clip.load_state_dict(synth.synth_clip_state_dict(cfg, seed=7), strict=True)
    return clip.to(dev).eval().visual.transformer.resblocks[0]


def alternate(fns, calls, warmup):
    """fns: {mode: callable}.  -> {mode: [ms per call]}; the modes take turns call by call"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    pairs = {m: [] for m in fns}
    for _ in range(calls):
        for m, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            pairs[m].append((a, b))
    torch.cuda.synchronize()
    return {m: [a.elapsed_time(b) for a, b in ev] for m, ev in pairs.items()}


def summary(ms):
    out = {m: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
           for m, v in ms.items()}
    out["fp32_over_bf16x3"] = round(out["fp32"]["median_ms"] / out["bf16x3"]["median_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--rows", type=int, default=1370)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    block = build_block(dev)
    L = a.rows
    aw = torch.nn.Parameter(synth._xavier("pbb.adapter", D, D, 31).to(dev), requires_grad=False)
    result = {"device": torch.cuda.get_device_name(0), "L": L, "D": D, "H": H, "F": F, "calls": a.calls,
              "warmup": a.warmup, "cases": {}}
    for B in a.batches:
        x = synth.randn("pbb.x", (B * L, D), 1.0, 31).to(dev)
        d_out = synth.randn("pbb.d", (B * L, D), 1.0, 31).to(dev)
        qkv = synth.randn("pbb.qkv", (B * L, 3 * D), 1.0, 31).to(dev)
        qkv[:, :D] *= 0.5
        if a.trace:
            for m in MODES:
                for _ in range(a.calls):
                    engine.block_backward(x, block, B, L, H, d_out, adapter_weight=aw, mix=0.1, precision=m)
            torch.cuda.synchronize()
            print("traced", a.calls, "calls per mode at B =", B)
            return
        for adapter in (True, False):
            fns = {m: (lambda m=m: engine.block_backward(x, block, B, L, H, d_out, adapter_weight=aw if adapter else None,
                                                         mix=0.1, precision=m)) for m in MODES}
            result["cases"][f"block.B{B}.{'adapter' if adapter else 'plain'}"] = summary(alternate(fns, a.calls, a.warmup))
        fns = {m: (lambda m=m: engine.attention_backward(qkv, d_out, B, L, H, False, dq_scale=0.125, precision=m))
               for m in MODES}
        result["cases"][f"attention_backward.B{B}"] = summary(alternate(fns, a.calls, a.warmup))
    line = json.dumps(result, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
