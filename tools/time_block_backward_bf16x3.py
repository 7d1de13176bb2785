"""engine.block_backward of one visual-tower block (L = 1370, D = 1024, 16 heads, F = 4096) in both backward
arithmetics, fp32 and bf16x3, in ONE process ("The bf16x3 backward").

Default: HIP-event timings.  For every (batch, adapter) it warms both modes up, then alternates fp32 / bf16x3 calls,
`--calls` each, every call between its own pair of events; the attention backward alone is timed the same way.  One JSON
line on stdout, the same object in --out.  The baseline is always the fp32 entry timed in this very run.

--compare A B C: no GPU.  A, B, C are --out files of three runs in ONE job on one box: a reference library (AACLIP_LIB),
the library under test, the reference again.  |A - C| is the noise of that box per median; `holds` says that no median
of B exceeds the larger of A's and C's by more than it.  Writes the three runs and the verdict to --out, exits 1 unless
`holds`.

--kernels A B: no GPU.  A, B are the kernel_trace.csv files of two `--trace --modes M` runs under rocprofv3, reference
library and library under test: per kernel the dispatches and the median duration of both, and their sum per call.

--trace: no timing, `--calls` calls per mode of `--modes` at the first batch with an adapter, for a
`rocprofv3 --kernel-trace --stats -- python tools/time_block_backward_bf16x3.py --trace` run (tracing only); the kernel
names tell the modes apart (attn_bwd_*_kernel<AttnBwdF32> against <AttnBwdBf16x3> and attn3_split_kernel, gemm32_kernel
against gemm16_kernel / the 256-tile kernels, split3_kernel)."""
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


def compare(paths, out):
    runs = [json.load(open(p)) for p in paths]
    doc = {k: runs[1][k] for k in ("device", "L", "D", "H", "F", "calls", "warmup")}
    doc.update(order="one job on one box: reference library, library under test, reference library again",
               rule="new median <= max(reference medians) + |reference_1 - reference_2| per case and mode",
               runs=dict(zip(("reference_1", "new", "reference_2"), (r["cases"] for r in runs))), median_ms={}, holds=True)
    for case in runs[1]["cases"]:
        for mode in MODES:
            a, b, c = (r["cases"][case][mode]["median_ms"] for r in runs)
            ok = b <= max(a, c) + abs(a - c)
            doc["median_ms"][f"{case}.{mode}"] = {"reference_1": a, "new": b, "reference_2": c, "noise": round(abs(a - c), 4),
                                                  "holds": ok}
            doc["holds"] = doc["holds"] and ok
            print(f"{case:26s} {mode:7s} reference {a:8.4f} {c:8.4f}  new {b:8.4f}  {'ok' if ok else 'SLOWER'}")
    print("holds", doc["holds"])
    if out:
        with open(out, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0 if doc["holds"] else 1


def kernels(paths, calls, out):
    """per kernel name (the pass kernels by their pass: before the skeleton they were attn3_* / attn_bwd_*) -> dispatches
    and median microseconds in both traces; `per_call_us` = sum of dispatches x median / calls"""
    import csv
    import re
    runs = []
    for p in paths:
        us = {}
        for row in csv.DictReader(open(p)):
            m = re.search(r"attn(3|_bwd)_(stats|dkv|dq)_kernel", row["Kernel_Name"])
            name = f"attn_bwd_{m.group(2)}_kernel" if m else row["Kernel_Name"]
            us.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        runs.append(us)
    doc = {"calls": calls, "kernels": {}, "per_call_us": {}}
    for name in sorted(set(runs[0]) | set(runs[1])):
        doc["kernels"][name] = {k: {"dispatches": len(r.get(name, [])), "median_us": round(statistics.median(r[name]), 3)
                                    if name in r else None} for k, r in zip(("reference", "new"), runs)}
    for k, r in zip(("reference", "new"), runs):
        doc["per_call_us"][k] = round(sum(len(v) * statistics.median(v) for v in r.values()) / calls, 2)
    text = json.dumps(doc, indent=1, sort_keys=True)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", nargs=2, metavar=("A", "B"))
    ap.add_argument("--modes", nargs="+", default=list(MODES), choices=MODES)
    ap.add_argument("--compare", nargs=3, metavar=("A", "B", "C"))
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--rows", type=int, default=1370)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(a.compare, a.out))
    if a.kernels:
        return kernels(a.kernels, a.calls, a.out)
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
            for m in a.modes:
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
