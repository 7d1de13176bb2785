"""Time of the bootstrap of one class's pixel AUROC / AP over its images (csrc/bootstrap.hip), R replicates, next to two
contenders on the same synthetic class, alternating in one process: N maps of 518 x 518 generated on the device, 3 %
positive pixels in every second image, with photographic-like scores (nearly every pixel its own tie group) and coarse
scores (256 levels: few groups).

  device    device-event time of engine.metrics_sort_pairs (the ONE sort) and of engine.bootstrap_curves (all replicates);
            `kernels`: the per-kernel device time of one bootstrap_curves call from the profiler's kernel records --
            pass 1 (bootstrap_walk_kernel<1>), scan, pass 2 (bootstrap_walk_kernel<2>), fold
  torch     (a) the same sums in torch on the same sorted arrays: per block of replicates a gather of the weights, two
            cumsums, the group terms as tensor expressions -- every replicate, device-event time; its records are compared
            with the kernels' (num / P / N equal, the largest AP difference)
  numpy     (b) forward_utils.bootstrap_eval, the definition, on 2 and on 6 replicates on the host; the time for R is
            EXTRAPOLATED from the two (the sort once, the rest per replicate) and labelled so
  harness   forward_utils.metrics_eval_device on the class with and without bootstrap=, alternating; the time without
            the keyword next to the committed profiles/metrics_device_timing.json of the same size

python tools/bench_bootstrap.py [--images 64 170] [--replicates 1000] [--rounds 2] [--out profiles/bootstrap_timing.json]"""
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


def make_class(n_img, kind, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    labels = np.arange(n_img) % 2
    anomalous = torch.from_numpy(labels).to(dev).view(-1, 1, 1, 1).bool()
    masks = ((torch.rand(n_img, 1, S, S, device=dev, generator=g) < 0.03) & anomalous).to(torch.uint8)
    maps = torch.randn(n_img, S, S, device=dev, generator=g) + 1.5 * masks[:, 0].float()
    if kind == "coarse":
        maps = torch.round(maps.clamp(-4, 6) * 25.5) / 25.5
    scores = torch.randn(n_img, device=dev, generator=g) + 1.2 * torch.from_numpy(labels).to(dev).float()
    return masks, labels, maps.contiguous(), scores


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0, a.elapsed_time(b) * 1e-3


def torch_bootstrap(keys, payload, counts, block=4):
    """contender (a): -> (num int64 [R], P, N, ap fp64 [R]) on the device"""
    n = keys.numel()
    image, lab = (payload >> 1).long(), (payload & 1)
    start = torch.ones(n, dtype=torch.bool, device=keys.device)
    start[1:] = keys[1:] != keys[:-1]
    i = torch.nonzero(start).view(-1)
    i2 = torch.cat([i[1:], torch.tensor([n], device=keys.device)])
    out = []
    for r0 in range(0, counts.shape[0], block):
        w = counts[r0:r0 + block].to(torch.int32)[:, image]                       # [b, n]
        zero = torch.zeros(w.shape[0], 1, dtype=torch.int64, device=keys.device)
        M = torch.cat([zero, torch.cumsum(w, dim=1, dtype=torch.int64)], dim=1)
        E = torch.cat([zero, torch.cumsum(w * lab, dim=1, dtype=torch.int64)], dim=1)
        del w
        P, Mt = E[:, -1:], M[:, -1:]
        tp, tp0 = P - E[:, i], P - E[:, i2]
        fp, fp0 = (Mt - M[:, i]) - tp, (Mt - M[:, i2]) - tp0
        del M, E
        num = ((fp - fp0) * (tp + tp0)).sum(dim=1)
        terms = ((tp - tp0).double() / P.double()) * (tp.double() / (tp + fp).double())
        ap = torch.where(tp == tp0, torch.zeros_like(terms), terms).sum(dim=1)
        out.append(torch.stack([num, P[:, 0], Mt[:, 0] - P[:, 0], ap.view(torch.int64)], dim=1))
        del tp, tp0, fp, fp0, terms
    return torch.cat(out)


def kernel_times(fn):
    """per-kernel device time (s) of one call of fn, from the profiler's kernel records; None where it records none"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.events():
            name = e.name
            if "bootstrap_" in name and getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0)):
                t = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0)
                key = ("pass1_s" if "walk_kernelILi1" in name or "walk_kernel<1>" in name else
                       "pass2_s" if "walk_kernel" in name else "scan_s" if "scan" in name else "fold_s")
                out[key] = out.get(key, 0.0) + t * 1e-6
        return out or None
    except Exception as e:   # the profiler is a convenience of this tool, not part of the measurement above it
        return {"error": repr(e)[:200]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[64, 170])
    ap.add_argument("--replicates", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--kinds", nargs="+", default=["photographic", "coarse"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bootstrap_timing.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    R = args.replicates
    record = {"device": torch.cuda.get_device_name(0), "map_size": S, "replicates": R, "rounds": args.rounds, "classes": []}
    parent = {}
    try:
        with open(os.path.join(ROOT, "profiles", "metrics_device_timing.json")) as f:
            parent = {c["images"]: c["device_metrics_eval_wall_s"] for c in json.load(f)["classes"]}
    except (OSError, ValueError, KeyError):
        pass
    for n_img in args.images:
        for kind in args.kinds:
            masks, labels, maps, scores = make_class(n_img, kind, dev, seed=n_img)
            n = maps.numel()
            counts = FU.bootstrap_counts(n_img, R, 0, 0)
            counts_dev = torch.from_numpy(counts).to(dev)
            rng, _ = engine.metrics_range(maps, masks.view(-1))
            norm = engine.metrics_normalise(maps.view(-1), rng)
            payload = ((torch.arange(n, dtype=torch.int32, device=dev) // (S * S)) << 1) | masks.view(-1).int()
            keys, carried = engine.metrics_sort_pairs(norm, payload)                 # warm-up, sizes the workspace
            engine.bootstrap_curves(keys, carried, counts_dev)
            sort_s, boot_s, torch_s = [], [], []
            equal, ap_diff = True, 0.0
            for r in range(args.rounds):
                (keys, carried), _, t = timed(lambda: engine.metrics_sort_pairs(norm, payload))
                sort_s.append(t)
                rec, _, t = timed(lambda: engine.bootstrap_curves(keys, carried, counts_dev))
                boot_s.append(t)
                ref, _, t = timed(lambda: torch_bootstrap(keys, carried, counts_dev))
                torch_s.append(t)
                valid = (rec[:, 1] > 0) & (rec[:, 2] > 0)
                equal = equal and bool(torch.equal(rec[valid][:, :3], ref[valid][:, :3]))
                ap_diff = max(ap_diff, float((rec[valid][:, 3].view(torch.float64) - ref[valid][:, 3].view(torch.float64))
                                             .abs().max()))
                del ref
                print(f"N={n_img} {kind} round {r}: sort {sort_s[-1]:.4f} s, bootstrap_curves {boot_s[-1]:.4f} s, torch "
                      f"{torch_s[-1]:.3f} s; records equal {equal}, worst |d ap| {ap_diff:.3g}", flush=True)
            kernels = kernel_times(lambda: engine.bootstrap_curves(keys, carried, counts_dev))
            groups = int((keys[1:] != keys[:-1]).sum()) + 1
            # (b) the numpy definition on a few replicates
            h_lab, h_norm = masks.view(-1).cpu().numpy(), norm.cpu().numpy()
            image_of = np.repeat(np.arange(n_img), S * S)
            numpy_s = {}
            for k in (2, 6):
                t0 = time.perf_counter()
                host = FU.bootstrap_eval(h_lab, h_norm, image_of, counts[:k])
                numpy_s[k] = time.perf_counter() - t0
            h = engine.bootstrap_records_host(rec[:6])
            numpy_equal = bool(np.array_equal(host.num, h.num) and np.abs(host.ap - h.ap).max() <= 1e-10)
            per_rep = (numpy_s[6] - numpy_s[2]) / 4
            del h_lab, h_norm, image_of
            entry = {
                "images": n_img, "pixels": n, "scores": kind, "tie_groups": groups,
                "invalid_replicates": int((~valid).sum()),
                "workspace_bytes": int(engine._lib.load().aaclip_bootstrap_workspace_bytes(n, n_img, R)),
                "device_sort_pairs_event_s": sort_s, "device_bootstrap_curves_event_s": boot_s,
                "device_bootstrap_kernels_s": kernels,
                "torch_cumsum_event_s": torch_s, "torch_records_equal": equal, "torch_worst_ap_diff": ap_diff,
                "torch_over_device": float(np.median(torch_s) / np.median(boot_s)),
                "numpy_definition_wall_s": {"2_replicates": numpy_s[2], "6_replicates": numpy_s[6]},
                "numpy_definition_equal_on_6": numpy_equal,
                "numpy_extrapolated_to_R_s": numpy_s[2] + (R - 2) * per_rep,
                "numpy_extrapolated_over_device": (numpy_s[2] + (R - 2) * per_rep) / float(np.median(boot_s) + np.median(sort_s))}
            if kind == args.kinds[0]:
                boot = dict(R=R, seed=0)
                FU.metrics_eval_device(masks, labels, maps, scores, "warm-up", "Industrial", bootstrap=boot)
                with_s, without_s = [], []
                for _ in range(3 * args.rounds):
                    _, wall, _ = timed(lambda: FU.metrics_eval_device(masks, labels, maps, scores, "c", "Industrial"))
                    without_s.append(wall)
                    row, wall, _ = timed(lambda: FU.metrics_eval_device(masks, labels, maps, scores, "c", "Industrial",
                                                                        bootstrap=boot))
                    with_s.append(wall)
                entry.update(metrics_eval_device_wall_s=without_s, metrics_eval_device_bootstrap_wall_s=with_s,
                             metrics_eval_device_wall_s_committed_before=parent.get(n_img), row=row)
                print(f"N={n_img}: metrics_eval_device {np.median(without_s):.4f} s, with bootstrap {np.median(with_s):.4f} s",
                      flush=True)
            record["classes"].append(entry)
            print(json.dumps(entry), flush=True)
            del masks, maps, scores, norm, payload, keys, carried, rec, counts_dev
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
