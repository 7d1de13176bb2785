"""Inputs and the fp64 / fp32 restatement of the stage-1 training step on the reduced model (reference train.py:62-100),
shared by tests/golden/make_golden_text_backward.py (which runs the reference's own AdaptedCLIP.encode_text,
calculate_similarity_map and calculate_seg_loss on them), tests/test_text_backward_cpu.py and
tests/test_gpu_text_backward.py.  Nothing at module level imports the build's packages, so the golden script can import
the reference's modules of the same names."""
import zlib

import torch

SEED = 20261017
E, GRID, IMG, BATCH = 256, 5, 70, 2
NORM_WEIGHT = 0.1            # text_norm_weight of the orthogonal term
SENTENCES = ["a photo of a flawless bottle.", "a photo of a damaged bottle."]     # column 0 normal, column 1 abnormal
ROW_STEP = 8                 # the golden keeps every 8th gradient row in fp64 (the whole tensors in fp32: file size)


def _gen(name: str) -> torch.Generator:
    return torch.Generator().manual_seed(SEED * 1000003 + zlib.crc32(name.encode()))


def patch_inputs(batch: int = BATCH, grid: int = GRID, img: int = IMG, width: int = E, name: str = "tb"):
    """-> (patch features [B, g*g, E]: unit rows + a unit cls row like train.py:82-85, mask [B, 1, S, S]) in fp64."""
    f = torch.randn(batch, grid * grid, width, generator=_gen(name + ".f"), dtype=torch.float64)
    f = f / f.norm(dim=-1, keepdim=True)
    cls = torch.randn(batch, 1, width, generator=_gen(name + ".cls"), dtype=torch.float64)
    f = f + cls / cls.norm(dim=-1, keepdim=True)
    mask = torch.zeros(batch, 1, img, img, dtype=torch.float64)
    for b in range(batch):
        y, x = 5 + 11 * b, 9 + 7 * b
        mask[b, 0, y:y + img // 3, x:x + img // 2] = 1
    return f, mask


def anchors(emb_normal: torch.Tensor, emb_abnormal: torch.Tensor) -> torch.Tensor:
    """reference forward_utils.py:154-161 -> [E, 2]"""
    cols = []
    for e in (emb_normal, emb_abnormal):
        e = e / e.norm(dim=-1, keepdim=True)
        m = e.mean(dim=0)
        cols.append(m / m.norm())
    return torch.stack(cols, dim=1)


def stage1_loss(text_feature: torch.Tensor, f: torch.Tensor, mask: torch.Tensor, img: int, norm_weight: float,
                similarity_map, seg_loss):
    """reference train.py:89-96 for one tap level: text_feature [B, E, 2]."""
    loss = seg_loss(similarity_map(f, text_feature, img), mask)
    orth = ((text_feature[:, :, 0] * text_feature[:, :, 1]).sum(1).mean()) ** 2
    return loss + orth * norm_weight


def oracle_loss(tokens_normal, tokens_abnormal, sd, ta, heads, until, f, mask, img, norm_weight, dtype):
    """The whole step on the CPU oracle in `dtype`; `ta` values may require grad.  -> loss"""
    import oracle.aaclip_oracle as O
    from seg_loss_cases import seg_loss_terms, similarity_map
    en = O.adapted_encode_text(tokens_normal, sd, ta, heads, text_adapt_until=until, dtype=dtype)
    ea = O.adapted_encode_text(tokens_abnormal, sd, ta, heads, text_adapt_until=until, dtype=dtype)
    t = anchors(en, ea).unsqueeze(0).expand(f.shape[0], -1, -1)
    return stage1_loss(t, f.to(dtype), mask.to(dtype), img, norm_weight, similarity_map,
                       lambda p, m: sum(seg_loss_terms(p, m)))
