"""Time of one optimizer step over the stage-2 parameter set of the full-size model: the trainable parameters of
AdaptedCLIP on ViT-L-14-336 with iqm_hidden_size 768 (105 tensors, 41.5 M elements, in the reference's two groups), with
synthetic values and gradients in place.  Only optimizer.step() is timed.  The candidates alternate in one process:

  torch        torch.optim.AdamW exactly as train.run constructs it (the step before aaclip_hip.optim existed)
  torch_fused  the same with torch's own fused=True, if this torch build accepts it
  fused        aaclip_hip.optim.FusedAdamW
  fused_clip   FusedAdamW(max_grad_norm=1.0): the norm over all parameters and the clipped step

Per candidate: wall time per step (host clock around `steps` steps that end in a synchronise) and device-event time per
step, medians over the rounds; for the library's candidates the bytes a step has to move (16 read + 12 written per
element, 4 more read per element with the norm) over the event time: a whole-step rate, launch gaps included.
Results: profiles/optim_step_timing.json.

Launches per step come from a kernel trace, in a run of its own (tracing slows the host, so its times are not used):

  rocprofv3 --kernel-trace --output-format csv -d <dir> -- python3 tools/bench_optim.py --trace_steps 5
  python3 tools/bench_optim.py --trace_dir <dir> --trace_steps 5 [--out profiles/optim_step_timing.json]

The traced run brackets every candidate's steps with three empty gradient-norm calls in a row (three consecutive
optim_norm_finish_kernel dispatches, which no step produces); the second command counts the dispatches between the
brackets and adds "launches_per_step", the kernel time per step and, for the library's candidates, the bytes over that
kernel time ("kernel_bytes_per_s") to the record.

python tools/bench_optim.py [--steps 20] [--rounds 5] [--out profiles/optim_step_timing.json]"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aa-clip-iqm_amd"))
from aaclip_hip import engine, optim  # noqa: E402

IMAGE_LR = 0.0005           # train.py's default --image_lr
MARK = "optim_norm_finish_kernel"


def parameter_shapes():
    """-> (image group shapes, IQM group shapes) of the full-size model, built on the meta device: no weights needed"""
    from model.adapter import AdaptedCLIP
    from model.clip import create_model
    with torch.device("meta"):
        clip = create_model(model_name="ViT-L-14-336", img_size=518, device="meta")
        model = AdaptedCLIP(clip_model=clip, iqm_hidden_size=768, relu=False)
    image = list(model.image_adapter.parameters())
    iqm = list(model.iqm.parameters()) + list(model.class_query_mlp.parameters()) + list(model.query_adapters.parameters())
    return [tuple(p.shape) for p in image], [tuple(p.shape) for p in iqm]


def make_params(shapes, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    params = []
    for shape in shapes:
        p = torch.nn.Parameter(torch.randn(shape, generator=gen, device=dev) * 0.02)
        p.grad = torch.randn(shape, generator=gen, device=dev) * 0.01
        params.append(p)
    return params


def candidates(dev):
    image_shapes, iqm_shapes = parameter_shapes()

    def groups():
        return [{"params": make_params(image_shapes, dev, 1), "lr": IMAGE_LR, "weight_decay": 1e-4},
                {"params": make_params(iqm_shapes, dev, 2), "lr": IMAGE_LR * 0.1, "weight_decay": 1e-3}]

    made = {"torch": torch.optim.AdamW(groups(), betas=(0.9, 0.999))}
    try:
        made["torch_fused"] = torch.optim.AdamW(groups(), betas=(0.9, 0.999), fused=True)
        made["torch_fused"].step()
    except (RuntimeError, ValueError, TypeError) as e:
        print("torch's fused=True is not available here:", e, flush=True)
        made.pop("torch_fused", None)
    made["fused"] = optim.FusedAdamW(groups(), betas=(0.9, 0.999))
    made["fused_clip"] = optim.FusedAdamW(groups(), betas=(0.9, 0.999), max_grad_norm=1.0)
    elements = sum(int(np.prod(s)) for s in image_shapes + iqm_shapes)
    return made, len(image_shapes) + len(iqm_shapes), elements


def mark(dev, record):
    for _ in range(3):
        engine.optim_grad_norm([], 1.0, record)


def traced_run(steps, dev):
    made, _, _ = candidates(dev)
    record = torch.zeros(engine.OPTIM_RECORD_FLOATS, device=dev)
    for opt in made.values():
        opt.step()                                       # state and workspaces exist before the brackets
    torch.cuda.synchronize()
    for name, opt in made.items():
        mark(dev, record)
        for _ in range(steps):
            opt.step()
        torch.cuda.synchronize()
    mark(dev, record)
    torch.cuda.synchronize()
    print("traced", list(made), "steps", steps)


def launches_from_trace(trace_dir, steps, names):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise RuntimeError(f"expected one *kernel_trace.csv under {trace_dir}, found {files}")
    with open(files[0]) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    kernels = [r["Kernel_Name"] for r in rows]
    spans = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9 for r in rows]
    sections, current, i = [], None, 0
    while i < len(kernels):
        if all(MARK in k for k in kernels[i:i + 3]) and len(kernels[i:i + 3]) == 3:
            if current is not None:
                sections.append(current)
            current, i = [], i + 3
            continue
        if current is not None:
            current.append((kernels[i], spans[i]))
        i += 1
    if len(sections) != len(names):
        raise RuntimeError(f"{len(sections)} bracketed sections in the trace, {len(names)} candidates")
    out = {}
    for name, section in zip(names, sections):
        by_kernel, seconds = {}, {}
        for k, span in section:
            short = k.split("(")[0][-60:]
            by_kernel[short] = by_kernel.get(short, 0) + 1
            seconds[short] = seconds.get(short, 0.0) + span
        out[name] = {"launches_per_step": len(section) / steps,
                     "kernel_s_per_step": sum(seconds.values()) / steps,
                     "kernels_per_step": {k: v / steps for k, v in sorted(by_kernel.items())},
                     "kernel_s_per_step_by_kernel": {k: v / steps for k, v in sorted(seconds.items())}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace_steps", type=int, default=0, help="run under rocprofv3 --kernel-trace: no timing")
    ap.add_argument("--trace_dir", default=None, help="count the launches of a traced run into the record at --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_step_timing.json"))
    args = ap.parse_args()
    if args.trace_dir:
        with open(args.out) as f:
            record = json.load(f)
        counted = launches_from_trace(args.trace_dir, args.trace_steps, list(record["candidates"]))
        for name, row in counted.items():
            record["candidates"][name].update(row)
            if "bytes_per_step" in record["candidates"][name]:      # the kernels alone, without the gaps between them
                record["candidates"][name]["kernel_bytes_per_s"] = (record["candidates"][name]["bytes_per_step"]
                                                                    / row["kernel_s_per_step"])
        record["launch_count_steps"] = args.trace_steps
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
        print(json.dumps({k: v["launches_per_step"] for k, v in counted.items()}))
        return
    if not torch.cuda.is_available():
        raise RuntimeError("tools/bench_optim.py measures on an MI355X; there is no CPU fallback")
    dev = torch.device("cuda:0")
    if args.trace_steps:
        return traced_run(args.trace_steps, dev)
    made, tensors, elements = candidates(dev)
    for opt in made.values():                            # warm-up: state, workspaces, code objects
        for _ in range(3):
            opt.step()
    torch.cuda.synchronize()
    wall = {k: [] for k in made}
    event = {k: [] for k in made}
    for r in range(args.rounds):
        for name, opt in made.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            for _ in range(args.steps):
                opt.step()
            b.record()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) / args.steps)
            event[name].append(a.elapsed_time(b) * 1e-3 / args.steps)
        print(f"round {r}: " + ", ".join(f"{k} wall {wall[k][-1] * 1e3:.3f} ms event {event[k][-1] * 1e3:.3f} ms"
                                         for k in made), flush=True)
    record = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "tensors": tensors,
              "elements": elements, "steps_per_round": args.steps, "rounds": args.rounds, "candidates": {}}
    bytes_per_element = {"fused": 28, "fused_clip": 32}
    for name in made:
        row = {"wall_s_per_step": wall[name], "event_s_per_step": event[name],
               "wall_s_median": float(np.median(wall[name])), "event_s_median": float(np.median(event[name]))}
        if name in bytes_per_element:
            row["bytes_per_step"] = bytes_per_element[name] * elements
            row["bytes_per_s"] = row["bytes_per_step"] / row["event_s_median"]
        record["candidates"][name] = row
    base = record["candidates"]["torch"]["wall_s_median"]
    record["fused_over_torch_wall"] = record["candidates"]["fused"]["wall_s_median"] / base
    record["fused_clip_over_torch_wall"] = record["candidates"]["fused_clip"]["wall_s_median"] / base
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print(json.dumps(record))


if __name__ == "__main__":
    main()
