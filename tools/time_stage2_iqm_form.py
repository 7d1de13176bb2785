#!/usr/bin/env python
"""Time one stage-2 training step (train.stage2_loss + backward) with the IQM branch trained in its projected form
against the folded 16-bit form (aaclip_hip.autograd.iqm_train_form), in one process on one MI355X.

The model is ViT-L-14-336 at image size 518 (L = 1370, D = 1024, four tap levels, IQM hidden size 768) with seeded
synthetic weights, precision fp16x2, no LeakyReLU: the configuration whose forward folds.  Batch 2 is the reference's
(train.py --batch_size).  Trainable: image_adapter, iqm, class_query_mlp, query_adapters (the reference's two optimizer
groups); no optimizer step is taken, so every step sees the same weights.

Method: both forms are warmed up, then timed in alternation (projected, folded, projected, ...) so that drift of the
shared host hits both alike; a step is timed with device events around forward + backward and ends in a synchronise;
peak memory is torch.cuda.max_memory_allocated over the step, reset before it (the caching allocator keeps the model and
the workspaces of earlier steps, so the figure is the model plus one step's live tensors).  Reported per form: median,
minimum and maximum step time over the rounds and the largest peak.  One JSON line on stdout.

    python tools/time_stage2_iqm_form.py [--batch 2] [--rounds 7] [--warmup 2]
"""
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


def build(dev, precision, image_size, hidden):
    from aaclip_hip import synth
    from model.adapter import AdaptedCLIP
    from model.clip import create_model
    cfg = synth.ClipCfg()
    clip = create_model("ViT-L-14-336", image_size, pretrained=None, precision=precision, force_image_size=image_size)
    clip.load_state_dict(synth.synth_clip_state_dict(cfg, 111), strict=True)
    model = AdaptedCLIP(clip, relu=False, iqm_hidden_size=hidden)
    model.image_adapter.load_state_dict(synth.synth_image_adapter_state_dict(cfg, seed=111), strict=True)
    model.load_state_dict(synth.synth_iqm_state_dict(cfg, hidden=hidden, seed=111), strict=False)
    for p in model.parameters():
        p.requires_grad_(False)
    for mod in (model.image_adapter, model.iqm, model.class_query_mlp, model.query_adapters):
        for p in mod.parameters():
            p.requires_grad_(True)
    return model.to(dev).eval()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--image_size", type=int, default=518)
    ap.add_argument("--precision", default="fp16x2")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_stage2_iqm_form: no GPU -- a step time is measured on an MI355X or not at all")
    import train
    from aaclip_hip import autograd, synth
    dev = torch.device("cuda:0")
    hidden = 768
    model = build(dev, args.precision, args.image_size, hidden)
    if not model.iqm_folds_levels():
        raise SystemExit("time_stage2_iqm_form: this model's forward does not fold")
    B, S = args.batch, args.image_size
    image = synth.synth_images(B, S, seed=7).to(dev)
    mask = torch.zeros(B, 1, S, S, device=dev)
    for b in range(B):
        mask[b, 0, 40 + 30 * b:40 + 30 * b + S // 3, 60 + 20 * b:60 + 20 * b + S // 2] = 1
    label = torch.arange(B, device=dev) % 2
    anchors = torch.nn.functional.normalize(synth.randn("time_stage2.anchors", (B, hidden, 2), 1.0, 7), dim=1).to(dev)

    def step(form):
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        with autograd.use_iqm_train_form(form):
            loss = train.stage2_loss(model, image, mask, label, anchors, S)
            loss.backward()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), torch.cuda.max_memory_allocated(), float(loss.detach())

    forms = ("projected", "folded")
    for _ in range(args.warmup):
        for f in forms:
            step(f)
    ms, peak, loss = {f: [] for f in forms}, {f: 0 for f in forms}, {}
    for _ in range(args.rounds):
        for f in forms:
            t, m, loss[f] = step(f)
            ms[f].append(t)
            peak[f] = max(peak[f], m)
    out = {"tool": "time_stage2_iqm_form", "device": torch.cuda.get_device_name(0), "precision": args.precision,
           "batch": B, "image_size": S, "rounds": args.rounds, "warmup": args.warmup}
    for f in forms:
        out[f] = {"step_ms_median": round(statistics.median(ms[f]), 3), "step_ms_min": round(min(ms[f]), 3),
                  "step_ms_max": round(max(ms[f]), 3), "peak_memory_mib": round(peak[f] / 2 ** 20, 1), "loss": loss[f]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
