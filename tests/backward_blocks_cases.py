"""Shapes, inputs, fp64 references and error bounds shared by tests/test_backward_blocks_cpu.py and
tests/test_gpu_backward_blocks.py: the fp32 building blocks of csrc/text_backward.hip, one at a time, judged per
element (gemm_wgrad, the LayerNorm / adapter-mix / head-normalize row kernels, the short attention backward, the
element-wise helpers through their callers, LeakyReLU's derivative at exactly zero).

Bounds.  An output element that the kernel forms as a sum of terms may be wrong by a multiple of 2^-24 times the sum
of the terms' absolute values (`terms`, formed in fp64 from the formula in the comment above the kernel):
    |got - ref| <= K * 2^-24 * terms.
K is one constant per kernel.  It is not taken from the kernel: the same formulas are evaluated with torch in fp32 on the
CPU, the largest ratio |fp32 - fp64| / (2^-24 * terms) over all cases is written down below (*_REF_RATIO) and K is 8
times that, the margin the project gives its kernels over the oracle's own fp32 error.  test_backward_blocks_cpu.py
recomputes the ratios and fails if a constant drops below what it was measured against.  The weight-gradient GEMM has a
derived bound instead (wgrad_bound)."""
import functools

import torch
import torch.nn.functional as F

import visual_backward_cases as VB
from aaclip_hip import synth

EPS24 = 2.0 ** -24
NONE, LEAKY, RELU = 0, 1, 2              # AACLIP_ACT_*
SLOPE = 0.01
WIDTHS = (256, 768, 1024)                # NCH = 1, 3, 4 of the row kernels
ROW_COUNTS = (1, 5, 131)                 # four rows per workgroup: less than one, one and a row, 32 and three rows
TAIL_ROWS = 4                            # sentinel rows behind every row-kernel buffer: a whole workgroup's worth


def rnd(name, shape, std=1.0):
    return synth.randn("bb." + name, shape, std, 31)


# ---------------------------------------------------------------------------------------------- gemm_wgrad
WGRAD_MAX_CHUNKS = 16


def wgrad_chunking(rows):
    """Plain copy of wgrad_chunking (csrc/text_backward.hip) -> (rows_per_chunk, chunks).

    rows    rows_per_chunk  chunks  what the row count is
       1          16           1    a single row: 15 of the 16 staged rows are zero fill
      15          16           1    one short of a K-step
      16          16           1    exactly one K-step
      17          32           1    one row into the second K-step
     128         128           1    the largest single chunk
     129          80           2    the first split (80 + 49 rows)
    2047         128          16    the 16-chunk cap from below (last chunk 127 rows)
    2048         128          16    the cap exactly
    2049         144          15    past the cap: FEWER chunks than the cap (14 x 144 + 33 rows)
    2176         144          16    144-row chunks, the last one a single K-step (16 rows)
    rows_per_chunk is always a multiple of 16, the K-step of wgrad_kernel: a K-step never straddles two chunks, so
    the kernel's row guard only ever cuts at `rows`."""
    nc = min(max((rows + 127) // 128, 1), WGRAD_MAX_CHUNKS)
    rpc = max(((rows + nc - 1) // nc + 15) // 16 * 16, 16)
    return rpc, (rows + rpc - 1) // rpc


WGRAD_ROWS = (1, 15, 16, 17, 128, 129, 2047, 2048, 2049, 2176)
WGRAD_TABLE = {r: wgrad_chunking(r) for r in WGRAD_ROWS}
# (rows, O, I): every row count with a non-square shape, every shape with a multi-chunk row count, O = I = 1024 (the
# documented limit of O) at 129 and 2049 only
WGRAD_CASES = [(1, 256, 1024), (15, 1024, 256), (16, 256, 1024), (17, 1024, 256), (128, 256, 1024), (128, 128, 128),
               (129, 1024, 256), (129, 256, 1024), (129, 128, 128), (129, 1024, 1024), (2047, 256, 1024),
               (2048, 1024, 256), (2049, 256, 1024), (2049, 1024, 1024), (2176, 1024, 256), (2176, 128, 128)]
WGRAD_EXACT_CASES = [(17, 1024, 256), (2049, 256, 1024)]           # single chunk, multi chunk; both non-square
WGRAD_STRIDED_CASES = [(1, 256, 1024), (17, 1024, 256), (129, 256, 1024), (2049, 1024, 256)]
WGRAD_PAD_Z, WGRAD_PAD_U = 4, 132        # ldz = O + 4, ldu = I + 132
WGRAD_OFF_Z, WGRAD_OFF_U = 4, 8          # first column of the window: 16 and 32 bytes into a buffer row


def wgrad_ws_floats(rows, O, I):
    rpc, nc = wgrad_chunking(rows)
    return nc * O * I if nc > 1 else 0


@functools.lru_cache(maxsize=None)
def wgrad_case(rows, O, I):
    """-> (dz [rows, O], u [rows, I] fp32, fp64 dz^T u, fp64 |dz|^T |u|): computed once, shared, never modified"""
    dz, u = rnd(f"wg.dz.{rows}.{O}.{I}", (rows, O)), rnd(f"wg.u.{rows}.{O}.{I}", (rows, I))
    return dz, u, dz.double().t() @ u.double(), dz.double().abs().t() @ u.double().abs()


def wgrad_bound(rows, mag):
    """(rows + 16) * 2^-24 * (|dz|^T |u|): one rounding per fused multiply-add of the `rows` products plus at most 16
    chunk additions gives the standard gamma bound, whatever the summation order."""
    return (rows + 16) * EPS24 * mag


@functools.lru_cache(maxsize=None)
def wgrad_exact_case(rows, O, I):
    """Small integers, asymmetric in both dimensions of both operands.  |dz| <= 13, |u| <= 6: every partial sum is
    below 2176 * 78 < 2^18, far inside 2^24, so any summation order is exact in fp32."""
    g = torch.Generator().manual_seed(1000 * rows + O + I)
    dz = torch.randint(-3, 4, (rows, O), generator=g).float()
    u = torch.randint(-2, 3, (rows, I), generator=g).float()
    dz += (torch.arange(rows).float() % 5)[:, None] * (torch.arange(O) % 3 == 0).float()[None, :]
    dz[0] += torch.arange(O).float() % 7
    u += (torch.arange(rows).float() % 3)[:, None] * (torch.arange(I) % 5 == 1).float()[None, :]
    u[-1] += torch.arange(I).float() % 3
    want = dz.double().t() @ u.double()
    assert float(dz.abs().max()) <= 13 and float(u.abs().max()) <= 6
    assert float((dz.double().abs().t() @ u.double().abs()).max()) < 2 ** 24
    return dz, u, want


# ---------------------------------------------------------------------------------------------- LayerNorm backward
# (D, rows, kind).  "plain": x ~ 2 N(0, 1) + 0.3, gamma = 1 + 0.1 N.  "edges": gamma ~ N(0, 1) (mixed signs) and, by
# row number modulo 4:  1 -> mean 50, std 0.1 (x - mean cancels six digits);  2 -> std 1e-4 about 0.5 (variance 1e-8,
# far below eps = 1e-5: rstd is eps^-1/2);  3 -> the constant 1.25 (variance exactly 0);  0 -> as in "plain".
LN_CASES = [(D, rows, kind) for D in WIDTHS for rows in ROW_COUNTS for kind in ("plain", "edges")]
LN_EPS = 1e-5


def ln_inputs(D, rows, kind):
    """-> x, gamma, beta, dy, d_resid (fp32)"""
    tag = f"ln.{D}.{rows}.{kind}."
    x = rnd(tag + "x", (rows, D), 2.0) + 0.3
    w = rnd(tag + "w", (D,), 0.1) + 1.0
    if kind == "edges":
        w = rnd(tag + "w", (D,), 1.0)
        assert (w > 0).any() and (w < 0).any()
        for r in range(rows):
            if r % 4 == 1:
                x[r] = rnd(tag + f"x{r}", (D,), 0.1) + 50.0
            elif r % 4 == 2:
                x[r] = rnd(tag + f"x{r}", (D,), 1e-4) + 0.5
            elif r % 4 == 3:
                x[r] = 1.25
    return x, w, rnd(tag + "b", (D,), 0.05), rnd(tag + "dy", (rows, D)), rnd(tag + "dr", (rows, D))


def ln_backward_formula(x, w, dy, add=None, eps=LN_EPS, g_terms=None):
    """The formula above ln_bwd_kernel in the dtype of its arguments -> (dx, terms):
    dx = rstd (g - mean g - xh mean(g xh)) [+ add], terms = rstd (|g| + |mean g| + |xh| |mean(g xh)|) [+ |add|].
    g_terms: the term sum of dy * w where dy itself is a computed sum (the heads), instead of |g|."""
    xc = x - x.mean(dim=-1, keepdim=True)
    rstd = torch.rsqrt((xc * xc).mean(dim=-1, keepdim=True) + eps)
    xh, g = xc * rstd, dy * w
    mg, mgx = g.mean(dim=-1, keepdim=True), (g * xh).mean(dim=-1, keepdim=True)
    dx = rstd * (g - mg - xh * mgx)
    terms = rstd * ((g.abs() if g_terms is None else g_terms) + mg.abs() + xh.abs() * mgx.abs())
    if add is not None:
        dx, terms = dx + add, terms + add.abs()
    return dx, terms


@functools.lru_cache(maxsize=None)
def ln_case(D, rows, kind):
    """-> (inputs, {"plain": (fp64 autograd dx, terms), "resid": (dx + d_resid, terms + |d_resid|)})"""
    x, w, b, dy, dr = ln_inputs(D, rows, kind)
    x64 = x.double().requires_grad_(True)
    F.layer_norm(x64, (D,), w.double(), b.double(), LN_EPS).backward(dy.double())
    _, t0 = ln_backward_formula(x.double(), w.double(), dy.double())
    return (x, w, b, dy, dr), {"plain": (x64.grad, t0), "resid": (x64.grad + dr.double(), t0 + dr.double().abs())}


def ln_fp32(D, rows, kind):
    """The same formulas in fp32 torch -> {"plain": dx, "resid": dx}"""
    x, w, b, dy, dr = ln_inputs(D, rows, kind)
    return {"plain": ln_backward_formula(x, w, dy)[0], "resid": ln_backward_formula(x, w, dy, dr)[0]}


# ---------------------------------------------------------------------------------------------- adapter-mix backward
# (D, rows, kind, mix).  "plain": u ~ 1.5 N, z ~ N.  "edges", by row number modulo 4:  0 -> every z negative (a = 0.01 z:
# the row lives on the small slope);  1 -> u scaled by 1e-3;  2 -> u scaled by 1e3;  3 -> as in "plain".  Squares stay
# between 1e-12 and 1e8: nothing underflows or overflows in fp32.  "zeros": exact zeros planted in z, +0.0 and -0.0, in
# every 256-column chunk and in a whole row of alternating signs of zero except one element (|a| must not vanish).
MIX_CASES = ([(D, rows, kind, mix) for D in WIDTHS for rows in ROW_COUNTS for kind, mix in (("plain", 0.1), ("edges", 0.9))]
             + [(D, 131, kind, mix) for D in WIDTHS for kind, mix in (("plain", 0.9), ("edges", 0.1))])
MIX_ZERO_CASES = [(D, rows, "zeros", mix) for D, rows, mix in ((256, 5, 0.1), (768, 131, 0.9), (1024, 5, 0.1))]


def mix_inputs(D, rows, kind, mix):
    """-> u, z, dy (fp32)"""
    tag = f"mix.{D}.{rows}.{kind}.{mix}."
    u, z, dy = rnd(tag + "u", (rows, D), 1.5), rnd(tag + "z", (rows, D)), rnd(tag + "dy", (rows, D))
    if kind == "edges":
        for r in range(rows):
            if r % 4 == 0:
                z[r] = -z[r].abs()
            elif r % 4 == 1:
                u[r] *= 1e-3
            elif r % 4 == 2:
                u[r] *= 1e3
    if kind == "zeros":
        pz, nz = torch.tensor(0.0), -torch.tensor(0.0)
        for r in range(rows):
            for c in range(D // 256):
                z[r, 256 * c + (7 * r + 3 * c) % 256] = pz if (r + c) % 2 else nz
        z[rows - 1, 0::2] = pz
        z[rows - 1, 1::2] = nz
        z[rows - 1, D - 3] = -0.75
        assert int((z == 0).sum()) >= (rows - 1) * (D // 256) + D - 1
        assert bool(torch.signbit(z[z == 0]).any()) and not bool(torch.signbit(z[z == 0]).all())
    assert float(z.abs().max()) > 0
    return u, z, dy


def mix_backward_formula(u, z, dy, mix):
    """The formulas above adapter_mix_bwd_kernel in the dtype of the arguments -> (dz, du, terms of dz, terms of du);
    LeakyReLU' = 1 for z > 0, 0.01 for z <= 0."""
    a = F.leaky_relu(z, SLOPE)
    nu, na = u.norm(dim=-1, keepdim=True), a.norm(dim=-1, keepdim=True)
    c = mix * (dy * a).sum(dim=-1, keepdim=True)
    k_u, k_dy, k_a = c / (na * nu), mix * nu / na, c * nu / (na * na * na)
    slope = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, SLOPE))
    dz = slope * (k_dy * dy - k_a * a)
    du = (1 - mix) * dy + k_u * u
    return dz, du, slope * (k_dy * dy.abs() + k_a.abs() * a.abs()), (1 - mix) * dy.abs() + k_u.abs() * u.abs()


@functools.lru_cache(maxsize=None)
def mix_case(D, rows, kind, mix):
    """-> (inputs, fp64 autograd (dz, du), fp64 (terms of dz, terms of du)); the reference is torch's leaky_relu."""
    u, z, dy = mix_inputs(D, rows, kind, mix)
    u64, z64 = u.double().requires_grad_(True), z.double().requires_grad_(True)
    a = F.leaky_relu(z64, SLOPE)
    y = mix * a * u64.norm(dim=-1, keepdim=True) / a.norm(dim=-1, keepdim=True) + (1 - mix) * u64
    y.backward(dy.double())
    _, _, t_dz, t_du = mix_backward_formula(u.double(), z.double(), dy.double(), mix)
    return (u, z, dy), (z64.grad, u64.grad), (t_dz, t_du)


def mix_fp32(D, rows, kind, mix):
    u, z, dy = mix_inputs(D, rows, kind, mix)
    return mix_backward_formula(u, z, dy, mix)[:2]


# ---------------------------------------------------------------------------------------------- the heads
# The head-normalize kernel has no entry point of its own: aaclip_tap_head_backward runs LayerNorm, the projection,
# head_norm_bwd_kernel on the projection rows z, the weight-gradient GEMM and (for d_x) the input-gradient product and
# the LayerNorm backward.  Per projection row, from the comment above the kernel: a = act(z), n = max(|a|, 1e-12),
# y = a / n,  dz = act'(z) (g - y <y, g>) / n  with terms  act'(z) (|g| + |y| |<y, g>|) / n.  The term sums of the
# outputs follow the products behind it:  d_w = dz^T ln -> terms(dz)^T |ln|;  d_ln = dz W -> terms(dz) |W|, which takes
# the place of |g| in the LayerNorm backward's term sum.
# name -> (B, L, D, E, act, zero_row).  Seg and det part and d_x, always.  zero_row: that row of proj_w and of det_w
# is zero, so that output feature's pre-activation is exactly 0 in every row.  The other pre-activations of a LEAKY case
# keep |z| > Z_MARGIN (they are computed in fp32; see head_backward_cases.py): head_case takes the first draw that does.
Z_MARGIN = 1e-5
HEAD_CASES = {}
for _D in WIDTHS:
    for _E in WIDTHS:
        HEAD_CASES[f"one_patch.{_D}.{_E}"] = (1, 2, _D, _E, NONE, None)        # rows = 2: half a workgroup
        HEAD_CASES[f"interleaved.{_D}.{_E}"] = (3, 5, _D, _E, LEAKY, None)     # 15 rows, CLS rows 0, 5, 10
HEAD_CASES["relu.768.1024"] = (3, 5, 768, 1024, RELU, None)
HEAD_ZERO_CASES = {
    "zero_row.256.256": (3, 5, 256, 256, LEAKY, 200),
    "zero_row.1024.768": (3, 5, 1024, 768, LEAKY, 700),
    "zero_row.768.1024": (1, 2, 768, 1024, LEAKY, 1023),
    "zero_row.relu.256.768": (3, 5, 256, 768, RELU, 5),
}
ALL_HEAD_CASES = dict(HEAD_CASES, **HEAD_ZERO_CASES)
HEAD_OUTPUTS = ("d_x", "d_proj_w", "d_det_w")


def head_inputs(name, draw):
    B, L, D, E, act, zero_row = ALL_HEAD_CASES[name]
    tag = f"head.{name}.{draw}."
    t = {"x": rnd(tag + "x", (B * L, D), 1.5) + 0.3, "ln_w": rnd(tag + "ln_w", (D,), 0.1) + 1.0,
         "ln_b": rnd(tag + "ln_b", (D,), 0.05), "proj_w": rnd(tag + "proj_w", (E, D), 1.3 * D ** -0.5),
         "det_w": rnd(tag + "det_w", (E, D), 1.3 * D ** -0.5), "d_seg": rnd(tag + "d_seg", (B, L - 1, E)),
         "d_det": rnd(tag + "d_det", (B, E))}
    if zero_row is not None:
        t["proj_w"][zero_row] = 0
        t["det_w"][zero_row] = 0
    return t


def act_forward(z, act):
    return F.leaky_relu(z, SLOPE) if act == LEAKY else torch.relu(z) if act == RELU else z


def act_slope(z, act):
    if act == LEAKY:
        return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, SLOPE))
    return (z > 0).to(z.dtype) if act == RELU else torch.ones_like(z)


def head_formula(t, B, L, act, terms=False):
    """The step sequence of aaclip_tap_head_backward in the dtype of t's tensors -> {d_x, d_proj_w, d_det_w} and, with
    terms=True, the term sums of the three as well."""
    x, lw, lb = t["x"], t["ln_w"], t["ln_b"]
    D = x.shape[1]
    xc = x - x.mean(dim=-1, keepdim=True)
    ln = xc * torch.rsqrt((xc * xc).mean(dim=-1, keepdim=True) + LN_EPS) * lw + lb
    patch = torch.ones(B, L, 1, dtype=x.dtype)
    patch[:, 0] = 0                                               # CLS rows: dz = 0
    out, tsum = {}, {}
    d_ln, t_dln = torch.zeros_like(x), torch.zeros_like(x)
    for key, w, det in (("d_proj_w", t["proj_w"], False), ("d_det_w", t["det_w"], True)):
        E = w.shape[0]
        z = ln @ w.t()
        g = torch.zeros(B, L, E, dtype=x.dtype)
        if det:
            g[:, 1:] = (t["d_det"] * (1.0 / (L - 1)))[:, None, :]
        else:
            g[:, 1:] = t["d_seg"]
        g = g.reshape(B * L, E)
        a = act_forward(z, act)
        n = a.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        y = a / n
        yg = (y * g).sum(dim=-1, keepdim=True)
        k = act_slope(z, act) * patch.reshape(B * L, 1) / n
        dz, t_dz = k * (g - y * yg), k * (g.abs() + y.abs() * yg.abs())
        out[key], tsum[key] = dz.t() @ ln, t_dz.t() @ ln.abs()
        d_ln, t_dln = d_ln + dz @ w, t_dln + t_dz @ w.abs()
    out["d_x"], tsum["d_x"] = ln_backward_formula(x, lw, d_ln, g_terms=t_dln * lw.abs())
    return (out, tsum) if terms else out


def _head_autograd(t, B, L, act):
    """fp64 torch autograd of layer_norm -> projection -> activation -> F.normalize (-> patch mean), both parts,
    contracted with d_seg / d_det -> ({d_x, d_proj_w, d_det_w}, smallest |z| over the rows that are not exactly zero)"""
    D = t["x"].shape[1]
    x = t["x"].double().reshape(B, L, D).requires_grad_(True)
    pw, dw = t["proj_w"].double().requires_grad_(True), t["det_w"].double().requires_grad_(True)
    ln = F.layer_norm(x, (D,), t["ln_w"].double(), t["ln_b"].double(), LN_EPS)[:, 1:, :]
    loss, zmin = 0, float("inf")
    for w, d, mean in ((pw, t["d_seg"].double(), False), (dw, t["d_det"].double(), True)):
        z = ln @ w.t()
        za = z.detach().abs()
        zmin = min(zmin, float(za[za > 0].min()))
        y = F.normalize(act_forward(z, act), dim=-1)
        loss = loss + ((y.mean(dim=1) if mean else y) * d).sum()
    loss.backward()
    return {"d_x": x.grad.reshape(B * L, D), "d_proj_w": pw.grad, "d_det_w": dw.grad}, zmin


@functools.lru_cache(maxsize=None)
def head_case(name):
    """-> (inputs, fp64 autograd gradients, fp64 term sums): computed once, shared, never modified"""
    B, L, D, E, act, zero_row = ALL_HEAD_CASES[name]
    for draw in range(50):
        t = head_inputs(name, draw)
        want, zmin = _head_autograd(t, B, L, act)
        if act == NONE or zmin > Z_MARGIN:
            break
    else:
        raise AssertionError(f"{name}: no draw keeps |z| above {Z_MARGIN}")
    t64 = {k: v.double() for k, v in t.items()}
    _, tsum = head_formula(t64, B, L, act, terms=True)
    if zero_row is not None:
        ln = F.layer_norm(t64["x"], (D,), t64["ln_w"], t64["ln_b"], LN_EPS)
        assert not (ln @ t64["proj_w"].t())[:, zero_row].any() and not (ln @ t64["det_w"].t())[:, zero_row].any()
    return t, want, tsum


def head_fp32(name):
    B, L, D, E, act, zero_row = ALL_HEAD_CASES[name]
    return head_formula(head_case(name)[0], B, L, act)


# aaclip_row_head_backward: pick a row per sequence, LayerNorm, projection, act' (ew_kernel<2>), weight gradient, and
# the LayerNorm backward scattered to the picked rows.  dz = act'(z) d_out has a single term.
# name -> (n, T, D, E, act, zero_row, picked row per sequence).  n E / 4 = 960 (no multiple of 256: the last workgroup of
# the element-wise kernel is cut by its guard), 256 and 256 (exact multiples).
ROW_HEAD_ZERO_CASES = {
    "zero_row.768.768": (5, 7, 768, 768, LEAKY, 300, (3, 6, 0, 4, 1)),
    "zero_row.1024.256": (4, 3, 1024, 256, LEAKY, 0, (2, 0, 1, 1)),
    "zero_row.256.1024": (1, 1, 256, 1024, LEAKY, 1023, (0,)),
}
ROW_HEAD_OUTPUTS = ("d_x", "d_proj_w")


def row_head_inputs(name, draw):
    n, T, D, E, act, zero_row, eot = ROW_HEAD_ZERO_CASES[name]
    tag = f"rowhead.{name}.{draw}."
    tokens = torch.randint(1, 1000, (n, T), generator=torch.Generator().manual_seed(D + E), dtype=torch.int32)
    for i, p in enumerate(eot):
        tokens[i, p] = 49407
    t = {"x": rnd(tag + "x", (n * T, D), 1.5), "ln_w": rnd(tag + "ln_w", (D,), 0.1) + 1.0,
         "ln_b": rnd(tag + "ln_b", (D,), 0.05), "proj_w": rnd(tag + "proj_w", (E, D), D ** -0.5),
         "d_out": rnd(tag + "d_out", (n, E)), "tokens": tokens}
    t["proj_w"][zero_row] = 0
    return t


def row_head_formula(t, name, terms=False):
    n, T, D, E, act, zero_row, eot = ROW_HEAD_ZERO_CASES[name]
    picked = torch.tensor([i * T + p for i, p in enumerate(eot)])
    x, lw, lb, w = t["x"][picked], t["ln_w"], t["ln_b"], t["proj_w"]
    xc = x - x.mean(dim=-1, keepdim=True)
    ln = xc * torch.rsqrt((xc * xc).mean(dim=-1, keepdim=True) + LN_EPS) * lw + lb
    dz = act_slope(ln @ w.t(), act) * t["d_out"]
    out = {"d_proj_w": dz.t() @ ln}
    tsum = {"d_proj_w": dz.abs().t() @ ln.abs()}
    dx, tx = ln_backward_formula(x, lw, dz @ w, g_terms=(dz.abs() @ w.abs()) * lw.abs())
    out["d_x"], tsum["d_x"] = torch.zeros_like(t["x"]), torch.zeros_like(t["x"])
    out["d_x"][picked], tsum["d_x"][picked] = dx, tx
    return (out, tsum) if terms else out


@functools.lru_cache(maxsize=None)
def row_head_case(name):
    """-> (inputs, fp64 autograd {d_x, d_proj_w}, fp64 term sums); the reference is torch's leaky_relu"""
    n, T, D, E, act, zero_row, eot = ROW_HEAD_ZERO_CASES[name]
    for draw in range(50):
        t = row_head_inputs(name, draw)
        x64, p64 = t["x"].double().requires_grad_(True), t["proj_w"].double().requires_grad_(True)
        rows = F.layer_norm(x64, (D,), t["ln_w"].double(), t["ln_b"].double(), LN_EPS)
        rows = rows.reshape(n, T, D)[torch.arange(n), torch.tensor(eot)]
        z = rows @ p64.t()
        za = z.detach().abs()
        assert not z.detach()[:, zero_row].any()
        if float(za[za > 0].min()) > Z_MARGIN:
            break
    else:
        raise AssertionError(name)
    act_forward(z, act).backward(t["d_out"].double())
    t64 = {k: (v.double() if v.is_floating_point() else v) for k, v in t.items()}
    _, tsum = row_head_formula(t64, name, terms=True)
    return t, {"d_x": x64.grad, "d_proj_w": p64.grad}, tsum


def row_head_fp32(name):
    return row_head_formula(row_head_case(name)[0], name)


# ---------------------------------------------------------------------------------------------- the measured constants
def ratio(got, want, terms):
    """Largest |got - want| / (2^-24 terms) over the elements; an element without terms must be exact."""
    err = (got.double() - want).abs()
    assert torch.isfinite(err).all()
    zero = terms == 0
    assert not err[zero].any(), "an element whose term sum is zero must be exactly right"
    return float((err[~zero] / (EPS24 * terms[~zero])).max()) if (~zero).any() else 0.0


def ln_ref_ratio():
    worst = 0.0
    for case in LN_CASES:
        want, got = ln_case(*case)[1], ln_fp32(*case)
        worst = max(worst, *(ratio(got[k], *want[k]) for k in ("plain", "resid")))
    return worst


def mix_ref_ratio():
    worst = 0.0
    for case in MIX_CASES + MIX_ZERO_CASES:
        _, want, terms = mix_case(*case)
        worst = max(worst, *(ratio(g, w, t) for g, w, t in zip(mix_fp32(*case), want, terms)))
    return worst


def head_ref_ratio():
    worst = 0.0
    for name in ALL_HEAD_CASES:
        _, want, terms = head_case(name)
        got = head_fp32(name)
        worst = max(worst, *(ratio(got[k], want[k], terms[k]) for k in HEAD_OUTPUTS))
    for name in ROW_HEAD_ZERO_CASES:
        _, want, terms = row_head_case(name)
        got = row_head_fp32(name)
        worst = max(worst, *(ratio(got[k], want[k], terms[k]) for k in ROW_HEAD_OUTPUTS))
    return worst


# Largest ratio of the fp32 torch evaluation of the formulas (ln_fp32, mix_fp32, head_fp32 / row_head_fp32) against the
# fp64 autograd references, over every case above.  *_REF_RATIO is the measured value times 1.1 (room for another BLAS's
# or another vector width's summation order on the CPU), rounded up to two digits; K = 8 x that.
#   LayerNorm backward   measured 2492.6  (the mean-50 rows: 1e3 times the other rows' 2 ... 20; the small-variance
#                                          and the constant rows reach 960 at width 1024)
#   adapter-mix backward measured 301.3
#   heads                measured 2326.4
LN_REF_RATIO = 2800.0
MIX_REF_RATIO = 340.0
HEAD_REF_RATIO = 2600.0
LN_K, MIX_K, HEAD_K = 8 * LN_REF_RATIO, 8 * MIX_REF_RATIO, 8 * HEAD_REF_RATIO


# ---------------------------------------------------------------------------------------------- short attention backward
ATTN_B, ATTN_H = 2, 3
ATTN_LENGTHS = (2, 63, 64, 65, 127)      # the kernel splits the keys as lane + 64 * jj: one short of, at and past 64
ATTN_PEAKED_LENGTHS = (65, 128)
ATTN_PEAK = 40.0                         # largest score of every row: most expf(s - m) of a row vanish
ATTN_CASES = ([(L, causal, None) for L in ATTN_LENGTHS for causal in (True, False)]
              + [(L, causal, ATTN_PEAK) for L in ATTN_PEAKED_LENGTHS for causal in (True, False)])
ATTN_WHOLE_BAR = 1e-4                    # the existing relative Frobenius bar over the whole output


@functools.lru_cache(maxsize=None)
def attention_case(L, causal, peak):
    """-> (qkv, d_ctx, fp64 d qkv): computed once, shared, never modified"""
    qkv, d_ctx = VB.attention_inputs(ATTN_B, ATTN_H, L, peak=peak)
    return qkv, d_ctx, VB.attention_reference(qkv, d_ctx, ATTN_B, ATTN_H, L, causal)


def attention_fp32(L, causal, peak):
    """torch autograd of softmax(q k^T) v in fp32 on the CPU -> d qkv"""
    qkv, d_ctx, _ = attention_case(L, causal, peak)
    D = 64 * ATTN_H
    x = qkv.clone().requires_grad_(True)
    q, k, v = (t.reshape(ATTN_B, L, ATTN_H, 64).transpose(1, 2) for t in x.split(D, dim=-1))
    s = q @ k.transpose(-1, -2)
    if causal:
        s = s + torch.triu(torch.full((L, L), float("-inf")), diagonal=1)
    (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(ATTN_B * L, D).backward(d_ctx)
    return x.grad


def segment_error(got, want, L):
    """The per-segment metric: for each of dq, dk, dv and every (b, head, row), the error norm of the 64-element segment
    over the largest reference segment norm of that kind within the (b, head) -> the largest of them.  (A relative error
    per segment would be meaningless: the causal row 0 has dq = 0 exactly.)"""
    shape = (ATTN_B, L, 3, ATTN_H, 64)
    err = (got.double().cpu() - want).reshape(shape).norm(dim=-1)          # [B, L, 3, H]
    top = want.reshape(shape).norm(dim=-1).amax(dim=1, keepdim=True)
    assert torch.isfinite(err).all() and (top > 0).all()
    return float((err / top).max())


def attention_ref_segment_error(L, peaked):
    """segment_error of attention_fp32 against fp64, the larger of the causal and the full case"""
    return max(segment_error(attention_fp32(*c), attention_case(*c)[2], L) for c in ATTN_CASES
               if c[0] == L and (c[2] is not None) == peaked)


# (L, peaked) -> attention_ref_segment_error times 1.1, rounded up to two digits (measured: 2.2763e-4, 1.6014e-6,
# 1.2441e-6, 1.1672e-6, 1.4545e-6; peaked 6.2408e-6, 6.1682e-6); the bar is 8 x that.  One entry per length, not one for
# all: at L = 2 a row's dq is p0 p1 (dp0 - dp1) (k0 - k1), a difference of two near-equal dot products, and plain fp32 is
# already 2e-4 off; a bar taken from that length would say nothing at the others.
ATTN_SEG_REF = {(2, False): 2.6e-4, (63, False): 1.8e-6, (64, False): 1.4e-6, (65, False): 1.3e-6, (127, False): 1.6e-6,
                (65, True): 6.9e-6, (128, True): 6.8e-6}


def attention_segment_bar(L, peak):
    return 8 * ATTN_SEG_REF[(L, peak is not None)]
