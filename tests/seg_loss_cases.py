"""Inputs of the training-loss fixtures (tests/golden/seg_loss.npz): patch features, text anchors and masks of the
stage-1 loss (reference train.py:76-100), each generated from a named seed.  Shared by
tests/golden/make_golden_seg_loss.py (which runs the reference's calculate_similarity_map(test=False) and
calculate_seg_loss on them), tests/test_seg_loss_cpu.py and tests/test_gpu_seg_loss.py.  Nothing here imports the
build's packages, so the golden script can import the reference's modules of the same names."""
import zlib

import torch

E = 768
SEED = 20261016
# name -> (B, g, S, mask kinds per image, shared anchors)
CASES = {
    "b1_g37_mixed": (1, 37, 518, ("rect",), False),
    "b4_g37_mixed": (4, 37, 518, ("zero", "one", "rect", "rect"), False),
    "b4_g5_zero": (4, 5, 33, ("zero",) * 4, False),
    "b4_g5_one": (4, 5, 33, ("one",) * 4, False),
    "b1_g5_mixed": (1, 5, 33, ("rect",), False),
    "b3_g5_shared": (3, 5, 33, ("rect", "zero", "rect"), True),
}
SEG_ROWS = 4   # rows of d(patch features) per image the golden keeps (p = 0, 1, ... spread over the grid)


def _gen(name: str) -> torch.Generator:
    return torch.Generator().manual_seed(SEED * 1000003 + zlib.crc32(name.encode()))


def seg_rows(P: int):
    return [int(round(i * (P - 1) / (SEG_ROWS - 1))) for i in range(SEG_ROWS)]


def make_case(name: str):
    """-> (patch features [B, g*g, E], anchors [B, E, 2] or [E, 2], mask [B, 1, S, S]) in fp64.  Patch rows are unit
    rows plus a unit cls row (train.py:84-92 adds the cls token without renormalising); anchor columns are unit
    means of unit rows, like _anchor."""
    B, g, S, kinds, shared = CASES[name]
    P = g * g
    f = torch.randn(B, P, E, generator=_gen(name + ".f"), dtype=torch.float64)
    f = f / f.norm(dim=-1, keepdim=True)
    cls = torch.randn(B, 1, E, generator=_gen(name + ".cls"), dtype=torch.float64)
    f = f + cls / cls.norm(dim=-1, keepdim=True)
    nb = 1 if shared else B
    base = torch.randn(nb, E, generator=_gen(name + ".t"), dtype=torch.float64)
    t = base.unsqueeze(-1) + 0.35 * torch.randn(nb, E, 2, generator=_gen(name + ".dt"), dtype=torch.float64)
    t = t / t.norm(dim=1, keepdim=True)
    if shared:
        t = t[0]
    mask = torch.zeros(B, 1, S, S, dtype=torch.float64)
    gm = _gen(name + ".mask")
    for b, kind in enumerate(kinds):
        if kind == "one":
            mask[b] = 1
        elif kind == "rect":
            y, x = (int(v) for v in torch.randint(0, S // 2, (2,), generator=gm))
            h, w = (int(v) for v in torch.randint(S // 8 + 1, S // 2, (2,), generator=gm))
            mask[b, 0, y:y + h, x:x + w] = 1
    return f, t, mask


# ---- fp64 restatement of the reference's math (forward_utils.py:21-108,196-227), differentiable through torch
def similarity_map(f, t, S):
    """calculate_similarity_map(test=False): 100 f.t -> [B, 2, g, g] -> bilinear align_corners -> softmax over 2."""
    s = 100.0 * torch.matmul(f, t)
    B, P, C = s.shape
    g = int(round(P ** 0.5))
    up = torch.nn.functional.interpolate(s.permute(0, 2, 1).reshape(B, C, g, g), size=S, mode="bilinear",
                                         align_corners=True)
    return torch.softmax(up, dim=1)


def seg_loss_terms(preds, mask):
    """-> (focal, dice(p0, 1 - m), dice(p1, m)); calculate_seg_loss is their sum in this order."""
    B = preds.shape[0]
    p = preds.reshape(B, 2, -1)
    m = mask.reshape(B, -1).to(p.dtype)
    k = m.long()
    oh1 = torch.where(k == 1, 1 - 1e-5, 1e-5).to(p.dtype)
    oh0 = torch.where(k == 0, 1 - 1e-5, 1e-5).to(p.dtype)
    pt = oh0 * p[:, 0] + oh1 * p[:, 1] + 1e-5
    focal = (-((1 - pt) ** 2) * torch.log(pt)).mean()

    def dice(x, tt):
        return 1 - ((2 * (x * tt).sum(1) + 1) / (x.sum(1) + tt.sum(1) + 1)).sum() / B

    return focal, dice(p[:, 0], 1 - m), dice(p[:, 1], m)
