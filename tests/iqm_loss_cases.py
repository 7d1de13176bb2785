"""Shapes, inputs and fp64 references shared by tests/test_iqm_loss_cpu.py and tests/test_gpu_iqm_loss.py
(aaclip_iqm_map_train and its backward, autograd.iqm_map_train, train.stage2_loss).

The reference is the restatement of reference train.py:173-212 in torch (F.cosine_similarity, torch.sigmoid, torch.cat,
F.interpolate(bilinear, align_corners=False)), differentiated by autograd.  It is only evaluated on non-degenerate
inputs: where |f|^2 |q|^2 <= 1e-16 torch clamps the two norms separately and the kernels clamp their product."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import head_backward_cases as HB
import oracle.aaclip_oracle as O
import visual_backward_cases as VB
from seg_loss_cases import seg_loss_terms, similarity_map
from visual_backward_cases import rnd

RANDOM, SUBSETS = "random", "subset means"
D_RANDOM, D_LOSS = "random", "seg loss of a rectangle mask"
P_SPAN = (0.3, 0.7)
# name -> (B, g, S, E, queries, d_preds)
IQM_CASES = {
    "one_patch": (3, 1, 7, 256, RANDOM, D_RANDOM),                  # one patch per image: every weight is 1
    "g5": (2, 5, 33, 256, SUBSETS, D_LOSS),
    "downsample": (2, 3, 2, 512, RANDOM, D_RANDOM),                 # S < g
    "same_size": (2, 6, 6, 256, RANDOM, D_LOSS),                    # S == g
    "production": (1, 37, 518, 768, SUBSETS, D_LOSS),               # P = 1369 is not a multiple of 4
    "largest_grid": (5, 40, 70, 1024, SUBSETS, D_RANDOM),           # chunked query sum, batch stride
}


def iqm_inputs(name):
    """-> dict of fp32 CPU tensors: seg [B, P, E] unit rows, queries [B, 2, E] of norm ~ sqrt(E) that differ per image,
    d_preds [B, 2, S, S] or None (D_LOSS: it is the loss's own gradient), mask [B, 1, S, S] or None.
    SUBSETS: q_abnormal = sqrt(E) unit(mean of two of the image's patch rows - mean of two others) + noise, q_normal the
    same with the two subsets swapped; the four rows then sit at z = cos - cos ~ +-1, so that p spans P_SPAN (random
    queries only give 0.46 .. 0.54 and barely exercise the sigmoid)."""
    B, g, S, E, qkind, dkind = IQM_CASES[name]
    P = g * g
    tag = f"iqm_loss.{name}."
    seg = rnd(tag + "seg", (B, P, E)).double()
    seg = (seg / seg.norm(dim=-1, keepdim=True)).float()
    if qkind == RANDOM:
        q = rnd(tag + "q", (B, 2, E))
    else:
        q = rnd(tag + "q", (B, 2, E), 0.1)
        for b in range(B):
            ia = [(3 * b) % P, (3 * b + P // 3) % P]
            ib = [(3 * b + P // 2) % P, (3 * b + (3 * P) // 4) % P]
            assert len(set(ia + ib)) == 4
            d = seg[b, ia].double().mean(0) - seg[b, ib].double().mean(0)
            d = (E ** 0.5 * d / d.norm()).float()
            q[b, 1] += d
            q[b, 0] -= d
    t = {"seg": seg, "queries": q, "d_preds": None, "mask": None}
    if dkind == D_RANDOM:
        t["d_preds"] = rnd(tag + "d_preds", (B, 2, S, S))
    else:
        mask = torch.zeros(B, 1, S, S)
        for b in range(B):
            y, x = S // 4 + b, S // 3 - b
            mask[b, 0, y:y + max(1, S // 3), x:x + max(1, S // 2)] = 1
        t["mask"] = mask
    return t


def iqm_map(seg, q, S):
    """reference train.py:185-209 -> (two-channel map [B, 2, S, S], p [B, P])"""
    norm_sim = F.cosine_similarity(seg, q[:, 0, :].unsqueeze(1), dim=-1)
    abnorm_sim = F.cosine_similarity(seg, q[:, 1, :].unsqueeze(1), dim=-1)
    p = torch.sigmoid(abnorm_sim - norm_sim)
    B, L = p.shape
    H = int(round(L ** 0.5))
    two = torch.cat([(1 - p).view(B, 1, H, H), p.view(B, 1, H, H)], dim=1)
    return F.interpolate(two, size=(S, S), mode="bilinear", align_corners=False), p


def iqm_reference(name, dtype):
    """The reference in `dtype` on the CPU -> dict(map, p, d_preds, d_seg, d_queries), detached"""
    B, g, S, E, _, dkind = IQM_CASES[name]
    t = iqm_inputs(name)
    seg = t["seg"].to(dtype).requires_grad_(True)
    q = t["queries"].to(dtype).requires_grad_(True)
    m, p = iqm_map(seg, q, S)
    if dkind == D_RANDOM:
        d_preds = t["d_preds"].to(dtype)
        (m * d_preds).sum().backward()
    else:
        m.retain_grad()
        sum(seg_loss_terms(m, t["mask"].to(dtype))).backward()
        d_preds = m.grad
    return {"map": m.detach(), "p": p.detach(), "d_preds": d_preds.detach(), "d_seg": seg.grad, "d_queries": q.grad}


@functools.lru_cache(maxsize=None)
def iqm_case(name):
    """-> (inputs with d_preds filled in as fp32, fp64 reference): computed once, shared, never modified"""
    t = iqm_inputs(name)
    want = iqm_reference(name, torch.float64)
    if IQM_CASES[name][4] == SUBSETS:
        lo, hi = float(want["p"].min()), float(want["p"].max())
        assert lo <= P_SPAN[0] and hi >= P_SPAN[1], f"{name}: p spans only {lo:.3f} .. {hi:.3f}"
    if t["d_preds"] is None:
        t["d_preds"] = want["d_preds"].float()
    return t, want


# ---- the kernels' half-pixel weight and support-window functions (csrc/iqm_loss.hip: hp_source, hp_weight,
# hp_support), mirrored in numpy at a chosen precision: np.float32 is the kernels' own arithmetic, np.float64 torch's
def hp_source(y, g, S, ft=np.float32):
    scale = ft(g) / ft(S)
    s = scale * (ft(y) + ft(0.5)) - ft(0.5)
    s = ft(0) if s < 0 else s
    i0 = int(s)
    i1 = i0 + (1 if i0 < g - 1 else 0)
    l1 = s - ft(i0)
    return i0, i1, ft(1) - l1, l1


def hp_weight(y, c, g, S, ft=np.float32):
    i0, i1, l0, l1 = hp_source(y, g, S, ft)
    return (l0 if i0 == c else ft(0)) + (l1 if i1 == c else ft(0))


def hp_support(c, g, S, ft=np.float32):
    scale = ft(g) / ft(S)
    lo = int(np.floor((ft(c) - ft(0.5)) / scale - ft(0.5))) - 1
    hi = int(np.ceil((ft(c) + ft(1.5)) / scale - ft(0.5))) + 1
    return max(lo, 0), min(hi, S - 1)


def hp_matrix(g, S, ft=np.float32, windowed=True):
    """W [S, g]: W[y, c] = weight of coarse index c at fine index y; windowed: only inside c's support window, as the
    backward kernels gather it"""
    W = np.zeros((S, g), dtype=np.float64)
    for c in range(g):
        lo, hi = hp_support(c, g, S, ft) if windowed else (0, S - 1)
        for y in range(lo, hi + 1):
            W[y, c] = float(hp_weight(y, c, g, S, ft))
    return W


# ---------------------------------------------------------------------------------------------- whole model
def stage2_queries():
    """[B, 2, E] fp32, norm ~ sqrt(E): stand-ins for the IQM branch's final queries on the reduced model"""
    return rnd("iqm_loss.stage2.queries", (VB.TAPS_BATCH, 2, 256))


def oracle_stage2_iqm(dtype):
    """head_backward_cases.oracle_stage2 with the IQM terms (reference train.py:152-212), in `dtype` on the CPU ->
    (loss, the IQM terms' share of it, gradients by HB.HEADS_KEYS, d queries)"""
    cfg, sd, ia, _ = HB.build_heads_model(torch.device("cpu"), "fp32")
    image, mask, anchors, label = HB.heads_inputs()
    leaves = {k: v.to(dtype) for k, v in ia.items()}
    for k in HB.HEADS_KEYS:
        leaves[k].requires_grad_(True)
    q = stage2_queries().to(dtype).requires_grad_(True)
    seg, det = O.adapted_visual_forward(image, sd, leaves, cfg.vision.heads, VB.TAPS_MIX, VB.TAPS_UNTIL, VB.TAPS_LEVELS,
                                        relu=False, dtype=dtype)
    a, m = anchors.to(dtype), mask.to(dtype)
    loss = 0.5 * F.cross_entropy(torch.matmul(det.unsqueeze(1), a)[:, 0], label)
    for s in seg:
        loss = loss + 0.6 * 0.5 * sum(seg_loss_terms(similarity_map(s, a, VB.TAPS_IMAGE), m))
    iqm = 0
    for s in seg:
        iqm = iqm + 0.4 * 0.5 * sum(seg_loss_terms(iqm_map(s, q, VB.TAPS_IMAGE)[0], m))
    loss = loss + iqm
    loss.backward()
    return loss.item(), float(iqm), {k: leaves[k].grad for k in HB.HEADS_KEYS}, q.grad


@functools.lru_cache(maxsize=None)
def oracle_stage2_iqm_fp64():
    return oracle_stage2_iqm(torch.float64)
