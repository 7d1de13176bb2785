"""Case tables and fp64 references for the C ABI entry points that are tested on their own at edge shapes: patch embed,
tap / keep-rows / det heads, row head, text embed, the two similarity maps and the attention lengths at the kernel
switches.  Shared by tests/test_entry_edges_cpu.py (which proves the references here against the oracle, torch and the
golden vectors) and tests/test_gpu_entry_edges.py (which compares the HIP kernels with them).  Plain torch on the CPU;
nothing here imports the build's GPU package.

Bars.  For patch embed, the heads and the row head the GPU tests assert max |got - ref| <= 4 x EMU_ERR[key], capped at
the file-level TOL of tests/test_gpu_parity.py.  EMU_ERR[key] is the maximum error, against the fp64 reference of the
same case, of a torch emulation of the mode's arithmetic (emu_* below): operands of the matrix product rounded to the
mode's format, products exact, fp32 accumulation with one rounding per K step of the MFMA instruction (2 for fp32, 16
for the 16-bit formats), fp32 LayerNorm / normalise with correctly rounded reductions.  The factor 4 covers another
summation order.  The fp64 reference takes the weight (patch embed: also the image) rounded to the mode's format, so
the figure is the error of the arithmetic, not of the operand format.
fp16x2 (split fp16, include/aaclip.h): its reference takes the fp32 operands (the mode exists to reproduce fp32), and
its emulation restates the split8 formats: A = fp16 + e4m3 correction, W likewise, product = Ah.Wh + Al8.Wh8 +
Ah8.Wl8.  For the heads and the row head the figure is the smaller of that and a quarter of plain fp16's.  For patch
embed plain fp16's figure holds no operand rounding at all (the reference rounds the image), so only the split
emulation applies there.
The figures are kept as constants (EMU_ERR); test_entry_edges_cpu.py recomputes them."""
import math
import zlib

import torch
import torch.nn.functional as F

from oracle import aaclip_oracle as O

SEED = 20261017
F32, F16, BF16, F16X2 = 0, 1, 2, 3          # include/aaclip.h
MODES = {"fp32": F32, "fp16": F16, "bf16": BF16, "fp16x2": F16X2}
ROW_WIDTHS = (256, 512, 768, 1024)          # csrc/rowops.hip row_width_check
# tests/test_gpu_parity.py TOL: the ceiling of every bar derived here
TOL = {"fp32": (2e-4, 1e-3), "fp16": (1e-3, 1e-2), "bf16": (1e-2, 5e-2), "fp16x2": (5e-4, 5e-3)}


def _gen(name: str) -> torch.Generator:
    return torch.Generator().manual_seed(SEED * 1000003 + zlib.crc32(name.encode()))


def randn(name: str, shape, std: float = 1.0, mean: float = 0.0) -> torch.Tensor:
    """fp32 normal values from a generator seeded by `name`"""
    return torch.randn(*shape, generator=_gen(name), dtype=torch.float32).mul_(std).add_(mean)


def rounded(t: torch.Tensor, mode: str) -> torch.Tensor:
    """fp64 value of t as the mode's matrix products see it (fp32 and fp16x2: the fp32 value)"""
    if mode == "fp16":
        return t.to(torch.float16).double()
    if mode == "bf16":
        return t.to(torch.bfloat16).double()
    return t.float().double()


# ----------------------------------------------------------------------------------------------------------------
# emulation of a mode's matrix product: operands in the mode's format, exact products, fp32 accumulation per K step
# ----------------------------------------------------------------------------------------------------------------
def _e4m3(v: torch.Tensor, exp: int) -> torch.Tensor:
    """fp64 value of e4m3(v * 2^exp) / 2^exp (OCP e4m3fn, clamped to +-448)"""
    s = float(2 ** exp)
    return (v.float() * s).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).double() / s


def emu_matmul(a: torch.Tensor, w: torch.Tensor, mode: str) -> torch.Tensor:
    """fp32 [M, N] = a [M, K] . w [N, K]^T (fp32 inputs) as the mode computes it"""
    a, w = a.float(), w.float()
    if mode == "fp16x2":      # split8 rows, include/aaclip.h: A = [hi | (v - hi) * 2^10 | v], W = [Wh | W * 2^6 | (W - Wh) * 2^17]
        ah, wh = a.to(torch.float16).double(), w.to(torch.float16).double()
        terms = [(ah, wh), (_e4m3(a - ah.float(), 10), _e4m3(w, 6)), (_e4m3(a, 0), _e4m3(w - wh.float(), 17))]
        step = 16
    else:
        terms = [(rounded(a, mode), rounded(w, mode))]
        step = 2 if mode == "fp32" else 16
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    for k in range(0, a.shape[1], step):
        part = sum(x[:, k:k + step] @ y[:, k:k + step].t() for x, y in terms)
        acc = (acc.double() + part).float()
    return acc


def emu_layer_norm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """fp32 LayerNorm: correctly rounded mean and variance, fp32 elementwise arithmetic"""
    x = x.float()
    mean = x.double().mean(-1, keepdim=True).float()
    d = x - mean
    var = d.double().pow(2).mean(-1, keepdim=True).float()
    rstd = (1.0 / (var + eps).double().sqrt()).float()
    return d * rstd * w.float() + b.float()


def emu_normalize(z: torch.Tensor) -> torch.Tensor:
    n = z.double().pow(2).sum(-1, keepdim=True).float().sqrt().clamp_min(1e-12)
    return z / n


def _act(z, act):
    return O.leaky_relu(z) if act else z


# ----------------------------------------------------------------------------------------------------------------
# 1. patch embed
# ----------------------------------------------------------------------------------------------------------------
# name -> (ps, H, W, D, modes); B = 2 everywhere.  K = 3 ps^2, Kpad = round_up(K, 64)
PATCH_B = 2
PATCH_CASES = {
    "a": (14, 28, 42, 256, ("fp32", "fp16", "bf16", "fp16x2")),   # K = 588 padded to 640
    "b": (14, 30, 45, 256, ("fp32", "fp16", "bf16", "fp16x2")),   # the floor: 2 surplus rows, 3 surplus columns
    "c": (8, 16, 8, 768, ("fp32", "fp16", "bf16")),               # K = 192 = Kpad
    "d": (2, 4, 6, 256, ("fp32", "fp16", "bf16")),                # K = 12 padded to 64
}
# (ps, H, W, D, mode): must return rc < 0 and leave the output untouched
PATCH_REJECTS = {"kpad_768": (16, 32, 32, 256, "fp32"), "fp16x2_kpad_192": (8, 16, 8, 768, "fp16x2")}


def patch_inputs(name: str):
    """-> img [B,3,H,W], conv1.weight [D,3,ps,ps], class_embedding [D], positional_embedding [L,D], ln_pre w, b"""
    ps, H, W, D = (PATCH_CASES.get(name) or PATCH_REJECTS[name])[:4]
    L = (H // ps) * (W // ps) + 1
    k = 3 * ps * ps
    return (randn(f"pe.{name}.img", (PATCH_B, 3, H, W), 1.2, 0.1), randn(f"pe.{name}.w", (D, 3, ps, ps), k ** -0.5),
            randn(f"pe.{name}.cls", (D,), 0.5), randn(f"pe.{name}.pos", (L, D), 0.3),
            randn(f"pe.{name}.lnw", (D,), 0.1, 1.0), randn(f"pe.{name}.lnb", (D,), 0.05))


def patch_embed_ref(img, conv_w, cls, pos, ln_w, ln_b, mode: str = "fp32") -> torch.Tensor:
    """reference model/adapter.py:139-156 in fp64 -> [B, L, D]; image and weight as the mode's product sees them"""
    ps = conv_w.shape[-1]
    y = F.conv2d(rounded(img, mode), rounded(conv_w, mode), stride=ps)             # [B, D, H/ps, W/ps]
    x = y.flatten(2).transpose(1, 2)
    x = torch.cat([cls.double().expand(x.shape[0], 1, -1), x], dim=1) + pos.double()
    return O.layer_norm(x, ln_w.double(), ln_b.double())


def patch_embed_emu(img, conv_w, cls, pos, ln_w, ln_b, mode: str) -> torch.Tensor:
    ps, D = conv_w.shape[-1], conv_w.shape[0]
    B, _, H, W = img.shape
    gh, gw = H // ps, W // ps
    cols = F.unfold(img[:, :, : gh * ps, : gw * ps], ps, stride=ps).transpose(1, 2).reshape(B * gh * gw, -1)
    y = emu_matmul(cols, conv_w.reshape(D, -1), mode).view(B, gh * gw, D) + pos[1:].float()
    x = torch.cat([(cls.float() + pos[0].float()).expand(B, 1, D), y], dim=1)
    return emu_layer_norm(x, ln_w, ln_b)


# ----------------------------------------------------------------------------------------------------------------
# 2. tap / keep-rows / det heads
# ----------------------------------------------------------------------------------------------------------------
# name -> (B, L, D, E, modes, acts)
HEAD_CASES = {
    "one_patch": (3, 2, 256, 256, ("fp32", "fp16", "bf16", "fp16x2"), (0,)),
    "ragged_slices": (2, 34, 256, 512, ("fp32", "fp16", "bf16", "fp16x2"), (0, 1)),   # 33 patches: rps 2, 17 slices
    # csrc/capi.hip ws_layout: narrow = rows * max(D, 640) * 2 bytes (fp16) = 2 * 34 * 640 * 2 = 87040 bytes = 21760
    # floats; launch_det_mean: fit = 21760 / (B * E = 2048) = 10 < 32 slices -> the clamp branch: rps = ceil(33 / 10) = 4,
    # 9 slices.  Without the clamp it would be rps 2 and 17 slices: the clamp changes the slice count here.  (This case
    # checks the clamped geometry's result; it does not claim that a missing clamp would be caught.)
    "clamped_slices": (2, 34, 256, 1024, ("fp16",), (0,)),
    "batch5": (5, 6, 1024, 768, ("fp32", "fp16", "bf16", "fp16x2"), (1,)),
}
HEAD_DEGENERATE = ("ragged_slices", 1, 5)   # (case, image, token row): every element 0.5, with ln_post bias zero


def head_inputs(name: str, degenerate: bool = False):
    """-> x [B, L, D] (CLS rows far from the patch rows), ln_post w, b, seg weight [E, D], det weight [E, D]"""
    B, L, D, E = HEAD_CASES[name][:4]
    x = randn(f"hd.{name}.x", (B, L, D), 1.5, 0.3)
    x[:, 0] = randn(f"hd.{name}.cls", (B, D), 40.0, 100.0)
    ln_w, ln_b = randn(f"hd.{name}.lnw", (D,), 0.1, 1.0), randn(f"hd.{name}.lnb", (D,), 0.05)
    if degenerate:
        assert name == HEAD_DEGENERATE[0]
        x[HEAD_DEGENERATE[1], HEAD_DEGENERATE[2]] = 0.5
        ln_b = torch.zeros(D)
    return x, ln_w, ln_b, randn(f"hd.{name}.w", (E, D), D ** -0.5), randn(f"hd.{name}.wd", (E, D), D ** -0.5)


def head_ref(x, ln_w, ln_b, w, wd, act: int, mode: str = "fp32"):
    """reference model/adapter.py:171-184 in fp64 -> (seg [B, L-1, E] unit rows, det [B, E])"""
    ln = O.layer_norm(x.double(), ln_w.double(), ln_b.double())
    seg = F.normalize(_act(ln @ rounded(w, mode).t(), act)[:, 1:], dim=-1)
    det = F.normalize(_act(ln @ rounded(wd, mode).t(), act)[:, 1:], dim=-1).mean(dim=1)
    return seg, det


def head_emu(x, ln_w, ln_b, w, wd, act: int, mode: str):
    B, L, D = x.shape
    ln = emu_layer_norm(x, ln_w, ln_b).view(B * L, D)
    seg = emu_normalize(_act(emu_matmul(ln, w, mode), act).view(B, L, -1)[:, 1:])
    det = emu_normalize(_act(emu_matmul(ln, wd, mode), act).view(B, L, -1)[:, 1:])
    return seg, det.double().mean(dim=1).float()


# ----------------------------------------------------------------------------------------------------------------
# 3. row head and text embed
# ----------------------------------------------------------------------------------------------------------------
ROW_T = 7
ROW_SHAPES = ((256, 256), (768, 768), (1024, 768))          # (D, E)
ROW_NS = (1, 3)
# token rows of mode 0 and the row each must pick (the FIRST maximum)
ROW_TOKENS = {"max_first": ([9, 1, 2, 3, 4, 5, 6], 0), "max_last": ([1, 2, 3, 4, 5, 6, 9], ROW_T - 1),
              "tie": ([1, 9, 2, 9, 3, 9, 5], 1), "all_equal": ([4] * ROW_T, 0)}
ROW_TOKEN_SETS = {1: (("max_first",), ("max_last",), ("tie",), ("all_equal",)),
                  3: (("max_first", "max_last", "tie"), ("all_equal", "tie", "max_last"))}


def row_inputs(D: int, E: int, n: int):
    """-> x [n, T, D]: every row its own direction and its own (large) scale, so that a neighbouring row gives
    another result in every mode; ln w, b; proj weight [E, D]"""
    x = randn(f"rh.{D}.{E}.{n}.x", (n, ROW_T, D), 1.0)
    x = x * (3.0 + 5.0 * torch.arange(n * ROW_T, dtype=torch.float32).view(n, ROW_T, 1)) + 2.0
    return x, randn(f"rh.{D}.lnw", (D,), 0.1, 1.0), randn(f"rh.{D}.lnb", (D,), 0.05), randn(f"rh.{D}.{E}.w", (E, D), D ** -0.5)


def row_tokens(names) -> torch.Tensor:
    return torch.tensor([ROW_TOKENS[k][0] for k in names], dtype=torch.int32)


def row_pick(tokens, n: int, mode_flag: int) -> torch.Tensor:
    """row index per sequence: mode 0 = first maximum of the token ids, mode 1 = row 0"""
    if mode_flag == 1:
        return torch.zeros(n, dtype=torch.long)
    return torch.stack([torch.tensor(int(torch.nonzero(r == r.max())[0])) for r in tokens.long()])


def row_head_ref(x, pick, ln_w, ln_b, w, act: int, mode: str = "fp32") -> torch.Tensor:
    """reference model/adapter.py:297-299 / model/transformer.py:542-546 in fp64 -> [n, E]"""
    ln = O.layer_norm(x.double(), ln_w.double(), ln_b.double())
    return _act(ln[torch.arange(x.shape[0]), pick] @ rounded(w, mode).t(), act)


def row_head_emu(x, pick, ln_w, ln_b, w, act: int, mode: str) -> torch.Tensor:
    ln = emu_layer_norm(x, ln_w, ln_b)
    return _act(emu_matmul(ln[torch.arange(x.shape[0]), pick], w, mode), act)


EMBED_VOCAB = 11
EMBED_SHAPES = ((2, 5, 4), (1, 3, 260), (3, 77, 768))       # (n, T, D)


def embed_inputs(n: int, T: int, D: int):
    """-> tokens [n, T] int32 holding ids 0 and vocab - 1, table [vocab, D], pos [T + 2, D]"""
    tok = torch.randint(0, EMBED_VOCAB, (n, T), generator=_gen(f"te.{n}.{T}.{D}.tok"), dtype=torch.int32)
    tok[0, 0], tok[-1, -1] = 0, EMBED_VOCAB - 1
    return tok, randn(f"te.{D}.table", (EMBED_VOCAB, D), 0.7), randn(f"te.{T}.{D}.pos", (T + 2, D), 0.3)


def embed_ref(tok, table, pos) -> torch.Tensor:
    """reference model/adapter.py:277-281: one fp32 add per element -> [n * T, D] fp32"""
    n, T = tok.shape
    return (table[tok.long()] + pos[:T]).reshape(n * T, -1)


# ----------------------------------------------------------------------------------------------------------------
# 4. maps
# ----------------------------------------------------------------------------------------------------------------
# name -> (B, g, S, E, NL, ksize, sigma, per-image anchors, index of the level scaled x30 or None)
MAP_CASES = {
    "g1_s1": (5, 1, 1, 256, 1, 1, 1.0, False, None),            # B * P = 5: not a multiple of 4 rows per workgroup
    "g1_s3": (5, 1, 3, 512, 2, 1, 1.0, False, None),
    "g1_s13": (2, 1, 13, 768, 4, 1, 1.0, True, None),
    "g1_s100": (3, 1, 100, 1024, 3, 1, 1.0, False, None),
    "g2_s1": (2, 2, 1, 1024, 1, 3, 1.0, False, None),           # ksize / 2 = g - 1
    "g2_s2": (3, 2, 2, 256, 3, 3, 0.8, False, None),            # S = g
    "g2_s3": (2, 2, 3, 768, 2, 1, 1.0, False, None),            # S = 2g - 1
    "g2_s13": (4, 2, 13, 512, 4, 3, 1.0, False, None),
    "g2_s100": (1, 2, 100, 256, 2, 1, 1.0, False, None),
    "g5_s1": (1, 5, 1, 768, 1, 9, 1.5, False, None),
    "g5_s3": (2, 5, 3, 512, 2, 3, 1.0, False, None),            # S < g
    "g5_s5_even": (2, 5, 5, 768, 1, 4, 1.0, False, None),       # even ksize, S = g
    "g5_s9_deep": (3, 5, 9, 1024, 4, 9, 1.5, True, None),       # reflection depth g - 1, S = 2g - 1
    "g5_s13": (2, 5, 13, 256, 3, 7, 1.0, False, None),          # fewer rows than the 14 bands
    "g5_s100_scaled": (2, 5, 100, 768, 4, 7, 1.0, False, 2),    # one level O(100), the others O(1)
    "g40_s1": (1, 40, 1, 256, 1, 15, 2.0, False, None),         # MAXG
    "g40_s3_even": (2, 40, 3, 512, 2, 4, 1.0, False, None),
    "g40_s13": (3, 40, 13, 256, 1, 3, 1.0, True, None),
    "g40_s40": (1, 40, 40, 768, 3, 15, 3.0, False, None),
    "g40_s79": (2, 40, 79, 1024, 4, 1, 1.0, False, None),
    "g40_s100": (2, 40, 100, 768, 4, 15, 2.5, True, None),
}
# name -> (g, NL, ksize, sigma, workspace bytes short): each must return rc < 0
MAP_REJECTS = {"g41": (41, 1, 3, 1.0, 0), "nl5": (5, 5, 3, 1.0, 0), "ksize16": (40, 1, 16, 1.0, 0),
               "half_ksize_ge_g": (2, 1, 5, 1.0, 0), "sigma0": (5, 1, 3, 0.0, 0), "ws_short": (5, 2, 3, 1.0, 1)}


def map_inputs(name: str):
    """-> (seg levels NL x [B, g*g, E] unit rows (one level x30 where the case says so), anchors [E,2] or [B,E,2])"""
    B, g, S, E, NL, ksize, sigma, per_image, scaled = MAP_CASES[name]
    segs = [F.normalize(randn(f"map.{name}.seg{l}", (B, g * g, E)), dim=-1) for l in range(NL)]
    if scaled is not None:
        segs[scaled] = segs[scaled] * 30.0
    t = F.normalize(randn(f"map.{name}.t", (B if per_image else 1, E, 2)), dim=1)
    return segs, (t if per_image else t[0])


def blur(m: torch.Tensor, ksize: int, sigma: float) -> torch.Tensor:
    """O.gaussian_blur2d; for an even ksize (which kornia, hence the reference, never takes, and whose padded
    convolution yields one row and column too many) the oracle's taps -- x = i - ksize/2 + 0.5 -- over the window
    [i - ksize/2, i + ksize/2 - 1], the HIP kernel's choice"""
    if ksize % 2:
        return O.gaussian_blur2d(m, ksize, sigma)
    B, C, H, W = m.shape
    k = O.gaussian_kernel1d(ksize, sigma, m.dtype)
    r = ksize // 2
    xp = F.pad(m, (r, r, r, r), mode="reflect").reshape(B * C, 1, H + 2 * r, W + 2 * r)
    xp = F.conv2d(F.conv2d(xp, k.view(1, 1, 1, ksize)), k.view(1, 1, ksize, 1))
    return xp[:, :, :H, :W].reshape(B, C, H, W)


def _scores(seg, anchors):
    s = 100.0 * torch.matmul(seg.double(), anchors.double())               # [B, P, 2]
    B, P, _ = s.shape
    g = math.isqrt(P)
    return s.permute(0, 2, 1).reshape(B, 2, g, g)


def anomaly_map_ref(segs, anchors, S: int, ksize: int, sigma: float) -> torch.Tensor:
    """calculate_similarity_map(test=True) per level for any (ksize, sigma), summed in level order -> [B, S, S]"""
    out = None
    for seg in segs:
        m = _scores(seg, anchors)
        m = ((m[:, 1] + 1 - m[:, 0]) / 2).unsqueeze(1)
        if ksize > 1:
            m = blur(m, ksize, sigma)
        m = O.bilinear_align_corners(m, S)[:, 0]
        out = m if out is None else out + m
    return out


def train_map_ref(seg, anchors, S: int) -> torch.Tensor:
    """calculate_similarity_map(test=False) -> [B, 2, S, S]"""
    return torch.softmax(O.bilinear_align_corners(_scores(seg, anchors), S), dim=1)


# ----------------------------------------------------------------------------------------------------------------
# 5. attention lengths at the kernel switches (csrc/attention.hip launch_attention)
# ----------------------------------------------------------------------------------------------------------------
ATTN_F32_L = (63, 64, 127, 128)                        # VALU kernel below 64, MFMA kernel from 64; one full query tile
ATTN_16_L = (128, 256, 257, 511, 512, 513, 576)        # the 512 switch, full 128- and 256-query tiles
ATTN_BATCHED = (3, 1, 513)                             # 9 tiles on a grid of 16 (16-bit), 15 on 16 (split)


def attn_inputs(B: int, L: int, H: int) -> torch.Tensor:
    """packed q|k|v rows [B*L, 3*H*64] with the scaling of tests/test_gpu_parity.py test_attention (logits O(5))"""
    qkv = randn(f"attn.{B}.{L}.{H}", (B * L, 3 * H * 64), 1.0)
    qkv[:, : H * 64] *= 0.6
    return qkv


def attn_ref(qkv, B, L, H, causal):
    D = H * 64
    q, k, v = qkv.double().view(B, L, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2)
    if causal:
        s = s + O.causal_mask(L, torch.float64)
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * L, D)


# ----------------------------------------------------------------------------------------------------------------
# emulation figures
# ----------------------------------------------------------------------------------------------------------------
def _maxerr(a, b) -> float:
    return float((a.double() - b.double()).abs().max())


def compute_emu_errors() -> dict:
    """key -> max |emulation - fp64 reference| over the case's inputs (every act of the case, every n of the row
    head); fp16x2 as the module docstring says"""
    out = {}
    for name, (ps, H, W, D, modes) in PATCH_CASES.items():
        args = patch_inputs(name)
        for mode in modes:
            out[f"patch.{name}.{mode}"] = _maxerr(patch_embed_emu(*args, mode), patch_embed_ref(*args, mode))
    for name, (B, L, D, E, modes, acts) in HEAD_CASES.items():
        args = head_inputs(name)
        raw = {}
        for mode in dict.fromkeys(modes + (("fp16",) if "fp16x2" in modes else ())):
            es = ed = 0.0
            for act in acts:
                (s, d), (rs, rd) = head_emu(*args, act, mode), head_ref(*args, act, mode)
                es, ed = max(es, _maxerr(s, rs)), max(ed, _maxerr(d, rd))
            raw[mode] = (es, ed)
        for mode in modes:
            es, ed = raw[mode]
            if mode == "fp16x2":
                es, ed = min(es, raw["fp16"][0] / 4), min(ed, raw["fp16"][1] / 4)
            out[f"head.{name}.{mode}.seg"], out[f"head.{name}.{mode}.det"] = es, ed
    for D, E in ROW_SHAPES:
        raw = {}
        for mode in MODES:
            e = 0.0
            for n in ROW_NS:
                x, lw, lb, w = row_inputs(D, E, n)
                picks = [row_pick(row_tokens(names), n, 0) for names in ROW_TOKEN_SETS[n]] + [row_pick(None, n, 1)]
                for pick in picks:
                    for act in (0, 1):
                        e = max(e, _maxerr(row_head_emu(x, pick, lw, lb, w, act, mode), row_head_ref(x, pick, lw, lb, w, act, mode)))
            raw[mode] = e
        for mode in MODES:
            out[f"row.{D}x{E}.{mode}"] = min(raw[mode], raw["fp16"] / 4) if mode == "fp16x2" else raw[mode]
    return out


def bar(key: str) -> float:
    """the GPU bar of a (entry point, case, mode): 4 x the emulation's error, capped at TOL's absolute part"""
    mode = next(m for m in ("fp16x2", "fp32", "fp16", "bf16") if f".{m}" in key)
    return min(4.0 * EMU_ERR[key], TOL[mode][0])


# computed by compute_emu_errors(); tests/test_entry_edges_cpu.py asserts that a recomputation still gives them
EMU_ERR = {
    "patch.a.fp32": 1.696e-06,
    "patch.a.fp16": 8.918e-07,
    "patch.a.bf16": 1.033e-06,
    "patch.a.fp16x2": 3.956e-05,
    "patch.b.fp32": 2.053e-06,
    "patch.b.fp16": 6.773e-07,
    "patch.b.bf16": 8.226e-07,
    "patch.b.fp16x2": 4.489e-05,
    "patch.c.fp32": 1.199e-06,
    "patch.c.fp16": 7.263e-07,
    "patch.c.bf16": 5.748e-07,
    "patch.d.fp32": 5.137e-07,
    "patch.d.fp16": 4.299e-07,
    "patch.d.bf16": 4.121e-07,
    "head.one_patch.fp32.seg": 7.147e-08,
    "head.one_patch.fp32.det": 1.002e-07,
    "head.one_patch.fp16.seg": 3.642e-05,
    "head.one_patch.fp16.det": 5.468e-05,
    "head.one_patch.bf16.seg": 3.450e-04,
    "head.one_patch.bf16.det": 3.314e-04,
    "head.one_patch.fp16x2.seg": 2.124e-06,
    "head.one_patch.fp16x2.det": 2.616e-06,
    "head.ragged_slices.fp32.seg": 1.144e-07,
    "head.ragged_slices.fp32.det": 6.559e-09,
    "head.ragged_slices.fp16.seg": 4.881e-05,
    "head.ragged_slices.fp16.det": 6.506e-06,
    "head.ragged_slices.bf16.seg": 4.427e-04,
    "head.ragged_slices.bf16.det": 5.391e-05,
    "head.ragged_slices.fp16x2.seg": 2.860e-06,
    "head.ragged_slices.fp16x2.det": 2.920e-07,
    "head.clamped_slices.fp16.seg": 2.843e-05,
    "head.clamped_slices.fp16.det": 3.837e-06,
    "head.batch5.fp32.seg": 1.334e-07,
    "head.batch5.fp32.det": 3.538e-08,
    "head.batch5.fp16.seg": 4.715e-05,
    "head.batch5.fp16.det": 1.340e-05,
    "head.batch5.bf16.seg": 3.619e-04,
    "head.batch5.bf16.det": 1.313e-04,
    "head.batch5.fp16x2.seg": 1.942e-06,
    "head.batch5.fp16x2.det": 6.976e-07,
    "row.256x256.fp32": 1.575e-06,
    "row.256x256.fp16": 8.125e-04,
    "row.256x256.bf16": 5.906e-03,
    "row.256x256.fp16x2": 4.065e-05,
    "row.768x768.fp32": 2.218e-06,
    "row.768x768.fp16": 8.507e-04,
    "row.768x768.bf16": 7.824e-03,
    "row.768x768.fp16x2": 4.102e-05,
    "row.1024x768.fp32": 2.632e-06,
    "row.1024x768.fp16": 7.805e-04,
    "row.1024x768.bf16": 9.531e-03,
    "row.1024x768.fp16x2": 4.690e-05,
}
