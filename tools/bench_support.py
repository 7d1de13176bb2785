#!/usr/bin/env python3
"""Time the few-shot support bank's nearest-patch search (csrc/support.hip, fp16 form) against what a user would write
instead -- torch.matmul of the fp16 rows in row chunks that fit memory, then .max(dim=1) -- on one MI355X, alternating
in one process; and against forward_utils.support_anomaly_map_host on this box's CPU.

  64 images x 4 tap levels, E = 768, K in {1, 4, 32} shots: per level M = 87 616 query rows, N = K * 1369 bank rows.

Reports per K: the time per level (median, min, max over the rounds), the achieved TFLOP/s (2 M N E over that time), that
rate as a share of the plain fp16 aaclip_gemm at the nearest shape tools/bench_gemm.py times (seg_proj: M = 64 * 1370,
N = 768, K = 1024, measured here in the same process), and the added time per 64-image evaluation step (4 levels) beside
the tower's (--tower_ms: ms_per_step of `bench.py --gpus 1`, taken in the same session).

usage: python tools/bench_support.py [--rounds 7] [--tower_ms MS] [--out profiles/support_timing.json] [--no-cpu]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "aa-clip-iqm_amd"))
import numpy as np
import torch

from aaclip_hip import _lib, engine

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=64)
ap.add_argument("--levels", type=int, default=4)
ap.add_argument("--shots", default="1,4,32")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--repeats", type=int, default=3, help="calls per timed window")
ap.add_argument("--tower_ms", type=float, default=None)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "support_timing.json"))
ap.add_argument("--no-cpu", action="store_true")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_support needs an MI355X; a CPU run measures nothing")
dev = torch.device("cuda:0")
lib = _lib.load()
P, E = 1369, 768
M = a.images * P


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


def unit_rows(n, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, E, generator=g), dim=-1)


q = unit_rows(M, 1).to(dev)
q16 = q.half()
result = {"device": torch.cuda.get_device_name(0), "images": a.images, "levels": a.levels, "patches": P, "E": E,
          "rounds": a.rounds, "repeats": a.repeats, "query_rows_per_level": M, "shots": []}

# the plain fp16 GEMM at the nearest shape of tools/bench_gemm.py (seg_proj), for the share
gM, gN, gK = a.images * 1370, 768, 1024
A = torch.randn(gM, gK, device=dev).half()
W = (torch.randn(gN, gK, device=dev) * gK ** -0.5).half()
bias = torch.randn(gN, device=dev)
gout = torch.zeros(gM, gN, device=dev)
st = torch.cuda.current_stream().cuda_stream


def run_gemm():
    _lib.check(lib.aaclip_gemm(_lib.F16, _lib.EPI_ACT_F32, A.data_ptr(), gK, W.data_ptr(), bias.data_ptr(), gout.data_ptr(),
                               gN, gM, gN, gK, 1, 0, 1.0, st))


for _ in range(3):
    run_gemm()
torch.cuda.synchronize()
gemm_ms = [timed(run_gemm, 10) for _ in range(a.rounds)]
gemm_tflops = 2.0 * gM * gN * gK / (statistics.median(gemm_ms) * 1e-3) / 1e12
result["aaclip_gemm_fp16_seg_proj"] = {"M": gM, "N": gN, "K": gK, "ms": spread(gemm_ms), "tflops": gemm_tflops}
print(f"aaclip_gemm fp16 seg_proj {gM}x{gN}x{gK}: {statistics.median(gemm_ms):.3f} ms, {gemm_tflops:.1f} TFLOP/s", flush=True)

for K in [int(v) for v in a.shots.split(",")]:
    N = K * P
    rows = unit_rows(N, 100 + K).to(dev)
    bank = engine.support_bank_rows(rows, "fp16")
    b16 = rows.half()
    chunk = min(M, max(1024, (1 << 29) // N))          # <= 1 GiB of fp16 cosines per chunk

    def fused():
        return engine.support_nearest(q, bank, want_idx=True)

    def torch_two_step(src=q16):
        best = torch.empty(M, dtype=torch.float16, device=dev)
        idx = torch.empty(M, dtype=torch.int64, device=dev)
        for r0 in range(0, M, chunk):
            v, i = torch.matmul(src[r0:r0 + chunk], b16.t()).max(dim=1)
            best[r0:r0 + chunk], idx[r0:r0 + chunk] = v, i
        return best, idx

    def torch_with_cast():
        return torch_two_step(q.half())

    # same results (the torch path rounds the cosine to fp16: 5e-4)
    c0, i0 = fused()
    c1, i1 = torch_two_step()
    torch.cuda.synchronize()
    agree = float((c0 - c1.float()).abs().max())
    for fn in (fused, torch_two_step, torch_with_cast):
        fn()
    torch.cuda.synchronize()
    t = {"fused": [], "torch": [], "torch_with_cast": []}
    for r in range(a.rounds):                          # the contenders alternate
        t["fused"].append(timed(fused, a.repeats))
        t["torch"].append(timed(torch_two_step, a.repeats))
        t["torch_with_cast"].append(timed(torch_with_cast, a.repeats))
    flop = 2.0 * M * N * E
    med = {k: statistics.median(v) for k, v in t.items()}
    entry = {"shots": K, "bank_rows": N, "flop_per_level": flop, "torch_chunk_rows": chunk,
             "cosine_matrix_bytes_fp32": 4.0 * M * N, "max_abs_difference_fused_vs_torch": agree,
             "ms_per_level": {k: spread(v) for k, v in t.items()},
             "tflops": {k: flop / (med[k] * 1e-3) / 1e12 for k in t},
             "fused_share_of_aaclip_gemm_rate": flop / (med["fused"] * 1e-3) / 1e12 / gemm_tflops,
             "torch_over_fused": med["torch"] / med["fused"],
             "added_ms_per_step": {k: a.levels * med[k] for k in t}}
    if a.tower_ms:
        entry["added_share_of_tower_step"] = {k: a.levels * med[k] / a.tower_ms for k in t}
    result["shots"].append(entry)
    print(f"K={K:2d} N={N}: fused {med['fused']:.3f} ms/level ({entry['tflops']['fused']:.0f} TFLOP/s, "
          f"{100 * entry['fused_share_of_aaclip_gemm_rate']:.0f} % of aaclip_gemm), torch {med['torch']:.3f} ms "
          f"({entry['tflops']['torch']:.0f} TFLOP/s), with cast {med['torch_with_cast']:.3f} ms; "
          f"added per step {entry['added_ms_per_step']['fused']:.2f} ms", flush=True)
    del rows, bank, b16
if a.tower_ms:
    result["tower_ms_per_step"] = a.tower_ms

if not a.no_cpu:
    import forward_utils as FU
    K = 4
    segs = [unit_rows(M, 10 + l).reshape(a.images, P, E).numpy() for l in range(a.levels)]
    banks = [unit_rows(K * P, 20 + l).reshape(K, P, E).numpy() for l in range(a.levels)]
    t0 = time.perf_counter()
    host = FU.support_anomaly_map_host(segs, banks, 518, "Industrial")
    host_s = time.perf_counter() - t0
    dsegs = [torch.from_numpy(s).to(dev) for s in segs]
    bank = engine.support_bank([[torch.from_numpy(b).to(dev) for b in banks]], "fp16")
    FU.support_anomaly_map(dsegs, bank, 518)
    torch.cuda.synchronize()
    dev_ms = [timed(lambda: FU.support_anomaly_map(dsegs, bank, 518), 3) for _ in range(a.rounds)]
    got = FU.support_anomaly_map(dsegs, bank, 518).cpu().numpy()
    result["map_64_images_4_shots"] = {"host_numpy_wall_s": host_s, "host_threads": torch.get_num_threads(),
                                       "device_ms": spread(dev_ms), "max_abs_difference": float(np.abs(got - host).max()),
                                       "host_over_device": host_s * 1e3 / statistics.median(dev_ms)}
    print(f"support map, 64 images x 4 levels, 4 shots: host numpy {host_s:.2f} s, device {statistics.median(dev_ms):.2f} ms", flush=True)

os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(result, f, indent=1)
print("wrote", a.out)
