"""Seeded cases and the fp64 reference shared by tests/test_cross_rows_levels_backward_cpu.py and
tests/test_gpu_cross_rows_levels_backward.py (aaclip_cross_rows_levels_backward).

The reference is the forward formula of aaclip_cross_rows_levels on the exact 16-bit row values,
    s_(r,s,j) = qt[b,r,s] . x[s][b,j],  p = softmax over all (s, j),  out[b,r,s] = sum_j p_(r,s,j) x[s][b,j],
differentiated by torch autograd in fp64."""
import functools

import torch

from aaclip_hip import synth

F16, BF16 = 1, 2                         # AACLIP_F16, AACLIP_BF16
MAX_SLICES = 128                         # csrc/kernels.h CRB_MAX_SLICES

# name -> dict(B, R, nseg, Lk, Dk) plus what departs from: fp16 rows of stride Dk, row0 = 0, rows_per_image = Lk,
# overwrite, both outputs, unit scores.  `peak`: every (b, r) is rescaled so that its largest score is `peak`.
# `ldx`: the row stride in elements (2 Dk: the fp16 halves of split8 rows; the other half holds values never read).
CASES = {
    "one_key": dict(B=1, R=4, nseg=1, Lk=1, Dk=768),                            # p = 1, ds = 0, d_qt = 0 exactly
    "two_segments_below_one_tile": dict(B=2, R=16, nseg=2, Lk=31, Dk=768),
    "two_segments_ragged": dict(B=2, R=16, nseg=2, Lk=33, Dk=768),
    "four_segments_bf16": dict(B=2, R=16, nseg=4, Lk=70, Dk=1024, code=BF16),
    "split8_r8": dict(B=2, R=8, nseg=3, Lk=70, Dk=768, ldx=2 * 768),
    "split8_r12": dict(B=2, R=12, nseg=2, Lk=45, Dk=1024, ldx=2 * 1024),
    "offset_rows": dict(B=3, R=16, nseg=2, Lk=36, Dk=768, row0=1, rows_per_image=37),
    "nearly_one_hot": dict(B=2, R=8, nseg=3, Lk=70, Dk=768, peak=80.0),
    "accumulate": dict(B=2, R=16, nseg=2, Lk=70, Dk=768, row0=1, rows_per_image=72, accumulate=True),
    "d_qt_only": dict(B=2, R=4, nseg=2, Lk=70, Dk=768, outs="d_qt"),
    "d_x_only": dict(B=2, R=4, nseg=2, Lk=70, Dk=768, outs="d_x"),
    "production": dict(B=2, R=16, nseg=4, Lk=1369, Dk=1024, row0=1, rows_per_image=1370),
}
SENTINEL = -7.25          # what the rows outside the key range hold before the call, and must hold after it


def rnd(name, shape, std=1.0):
    return synth.randn("clb." + name, shape, std, 37)


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.isfinite(a).all()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def dims(name):
    """-> (B, R, nseg, Lk, Dk, rows_per_image, row0, ldx, code)"""
    c = CASES[name]
    return (c["B"], c["R"], c["nseg"], c["Lk"], c["Dk"], c.get("rows_per_image", c["Lk"]), c.get("row0", 0),
            c.get("ldx", c["Dk"]), c.get("code", F16))


def key_rows(buf, name, width=None):
    """the key rows of one level buffer [B*rows_per_image, >= Dk] -> [B, Lk, Dk]"""
    B, _, _, Lk, Dk, rpi, row0, _, _ = dims(name)
    return buf.view(B, rpi, -1)[:, row0:row0 + Lk, :width or Dk]


def case_inputs(name):
    """-> dict: qt, d_out [B*R, nseg*Dk] fp32; x: per level [B*rows_per_image, ldx] in the case's 16-bit dtype; base: per
    level [B*rows_per_image, Dk] fp32 (accumulate cases)"""
    c = CASES[name]
    B, R, nseg, Lk, Dk, rpi, row0, ldx, code = dims(name)
    dt = torch.float16 if code == F16 else torch.bfloat16
    x = [rnd(f"{name}.x{s}", (B * rpi, ldx)).to(dt) for s in range(nseg)]
    qt = rnd(name + ".qt", (B * R, nseg * Dk), 1.5 * Dk ** -0.5)
    if c.get("peak") is not None:
        s = scores(qt.double(), [key_rows(v, name).double() for v in x], B, R, nseg, Dk)
        qt = (qt.double().view(B, R, -1) * (c["peak"] / s.amax(dim=-1, keepdim=True))).view(B * R, -1).float()
    t = {"qt": qt, "x": x, "d_out": rnd(name + ".d_out", (B * R, nseg * Dk))}
    if c.get("accumulate"):
        t["base"] = [rnd(f"{name}.base{s}", (B * rpi, Dk), 0.05) for s in range(nseg)]
    return t


def scores(qt, xs, B, R, nseg, Dk):
    """qt [B*R, nseg*Dk], xs: per level [B, Lk, Dk] -> [B, R, nseg*Lk], segment-major"""
    q = qt.view(B, R, nseg, Dk)
    return torch.cat([q[:, :, s, :] @ xs[s].transpose(1, 2) for s in range(nseg)], dim=-1)


def autograd_reference(name, t, dtype=torch.float64):
    """-> (d_qt [B*R, nseg*Dk], [d_x[s] [B, Lk, Dk]], out [B*R, nseg*Dk]) of the forward formula in `dtype` on the CPU"""
    B, R, nseg, Lk, Dk = dims(name)[:5]
    q = t["qt"].detach().to(dtype).clone().requires_grad_(True)
    xs = [key_rows(v, name).to(dtype).contiguous().requires_grad_(True) for v in t["x"]]
    p = torch.softmax(scores(q, xs, B, R, nseg, Dk), dim=-1).view(B, R, nseg, Lk)
    out = torch.stack([p[:, :, s, :] @ xs[s] for s in range(nseg)], dim=2).reshape(B * R, nseg * Dk)
    out.backward(t["d_out"].to(dtype))
    return q.grad, [v.grad for v in xs], out.detach()


def want_of(name, d_qt, d_x, t):
    """what the entry point is to leave in d_qt and in the KEY ROWS of every d_x[s], from the plain gradients"""
    c = CASES[name]
    if c.get("accumulate"):
        d_x = [key_rows(b, name).to(g.dtype) + g for b, g in zip(t["base"], d_x)]
    outs = c.get("outs", "both")
    return {"d_qt": d_qt if outs != "d_x" else None, "d_x": torch.stack(d_x) if outs != "d_qt" else None}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (inputs, fp64 expectations {d_qt [B*R, nseg*Dk], d_x [nseg, B, Lk, Dk]}): computed once, shared, never
    modified"""
    t = case_inputs(name)
    d_qt, d_x, _ = autograd_reference(name, t)
    return t, want_of(name, d_qt, d_x, t)


def step_sequence(name, t):
    """The passes of csrc/iqm_levels_backward.hip in fp64 torch -> (d_qt [B*R, nseg*Dk], [d_x[s] [B, Lk, Dk]])"""
    B, R, nseg, Lk, Dk = dims(name)[:5]
    q, do = (v.double().view(B, R, nseg, Dk) for v in (t["qt"], t["d_out"]))
    xs = [key_rows(v, name).double() for v in t["x"]]
    # scores pass: per segment [B, Lk, R]; one record list per image over all segments
    S = torch.cat([xs[s] @ q[:, :, s, :].transpose(1, 2) for s in range(nseg)], dim=1)
    G = torch.cat([xs[s] @ do[:, :, s, :].transpose(1, 2) for s in range(nseg)], dim=1)
    m = S.amax(dim=1, keepdim=True)                                   # ONE set of statistics over all segments
    e = torch.exp(S - m)
    linv = 1.0 / e.sum(dim=1, keepdim=True)
    delta = (e * linv * G).sum(dim=1, keepdim=True)
    P = e * linv                                                      # gradient pass, per segment
    dS = P * (G - delta)
    d_x, d_qt = [], []
    for s in range(nseg):
        ps, ds = P[:, s * Lk:(s + 1) * Lk], dS[:, s * Lk:(s + 1) * Lk]
        d_x.append(torch.cat([ps, ds], dim=2) @ torch.cat([do[:, :, s, :], q[:, :, s, :]], dim=1))
        d_qt.append(ds.transpose(1, 2) @ xs[s])
    return torch.stack(d_qt, dim=2).reshape(B * R, nseg * Dk), d_x
