"""Text anchors and similarity maps with the reference's function names
(reference forward_utils.py:138-216), executed by the HIP path."""
from __future__ import annotations

import collections
from typing import Sequence

import torch

from aaclip_hip import _lib, autograd, engine
from dataset.constants import CLASS_NAMES, DOMAINS, PROMPTS, REAL_NAMES  # noqa: F401  (DOMAINS: re-exported like the reference)
from model.tokenizer import tokenize

prompt_normal = PROMPTS["prompt_normal"]
prompt_abnormal = PROMPTS["prompt_abnormal"]
prompt_state = [prompt_normal, prompt_abnormal]
prompt_templates = PROMPTS["prompt_templates"]


def class_sentences(dataset_name: str, class_name: str):
    """The 6 normal + 10 abnormal sentences of one class (forward_utils.py:139-152)."""
    if class_name == "object":
        real_name = class_name
    else:
        assert class_name in CLASS_NAMES[dataset_name], (
            f"class_name {class_name} not found; available class_names: {CLASS_NAMES[dataset_name]}")
        real_name = REAL_NAMES[dataset_name][class_name]
    return [[tpl.format(state.format(real_name)) for state in states for tpl in prompt_templates]
            for states in prompt_state]


def _anchor(embeddings: torch.Tensor) -> torch.Tensor:
    # [n, E] sentence embeddings -> unit mean of unit rows (forward_utils.py:155-159); n <= 10 rows, host-side math
    e = embeddings / embeddings.norm(dim=-1, keepdim=True)
    m = e.mean(dim=0)
    return m / m.norm()


def get_adapted_single_class_text_embedding(model, dataset_name, class_name, device):
    """-> [E, 2]: column 0 normal, column 1 abnormal (forward_utils.py:138-162)."""
    cols = []
    for sentences in class_sentences(dataset_name, class_name):
        tokens = tokenize(sentences).to(device)
        cols.append(_anchor(model.encode_text(tokens)))
    return torch.stack(cols, dim=1).to(device)


def get_adapted_text_embedding(model, dataset_name, device):
    """dict class -> [E, 2] (forward_utils.py:185-192).  All classes x states go
    through ONE batched encode_text call (the tiny M = n*77 GEMMs are launch-bound
    one class at a time), then a segmented mean."""
    names = list(CLASS_NAMES[dataset_name])
    groups, sentences = [], []
    for c in names:
        for s in class_sentences(dataset_name, c):
            groups.append((c, len(sentences), len(s)))
            sentences.extend(s)
    emb = model.encode_text(tokenize(sentences).to(device))
    out = {}
    for c in names:
        cols = [_anchor(emb[start:start + n]) for (cc, start, n) in groups if cc == c]
        out[c] = torch.stack(cols, dim=1).to(device)
    return out


def calculate_similarity_map(patch_features, epoch_text_feature, img_size, test=False, domain="Medical"):
    """forward_utils.py:196-216.  test=True -> [B,1,S,S] blurred/upsampled anomaly
    map; test=False -> [B,2,S,S] softmax over the two anchors."""
    if test:
        assert epoch_text_feature.shape[-1] == 2
        sigma, ksize = (1.0, 7) if domain == "Industrial" else (1.5, 9)
        return engine.anomaly_map([patch_features], epoch_text_feature, img_size, ksize, sigma).unsqueeze(1)
    if torch.is_grad_enabled() and (patch_features.requires_grad or epoch_text_feature.requires_grad):
        return autograd.similarity_map_train(patch_features, epoch_text_feature, img_size)   # same forward kernels
    return engine.similarity_map_train(patch_features, epoch_text_feature, img_size)


# ------------------------------------------------------------------------------------------------
# training criterion (reference forward_utils.py:21-108,223-227): one HIP loss kernel pair, differentiable in preds
class FocalLoss(torch.nn.Module):
    """The reference's FocalLoss as train.py uses it (apply_nonlin None, alpha None = 1, gamma 2, smooth 1e-5,
    size_average): mean over pixels of -(1 - pt)^2 log pt on 2-channel probabilities [B,2,S,S] and a 0/1 mask."""

    def __init__(self, apply_nonlin=None, alpha=None, gamma=2, balance_index=0, smooth=1e-5, size_average=True):
        super().__init__()
        if apply_nonlin is not None or alpha is not None or gamma != 2 or smooth != 1e-5 or not size_average:
            raise NotImplementedError("FocalLoss: the HIP kernel implements the configuration calculate_seg_loss uses "
                                      "(apply_nonlin=None, alpha=None, gamma=2, smooth=1e-5, size_average=True)")
        self.gamma, self.smooth = gamma, smooth

    def forward(self, logit, target):
        return autograd.seg_loss(logit, target, _lib.SEG_LOSS_FOCAL)[1]


class BinaryDiceLoss(torch.nn.Module):
    """1 - mean over images of (2 sum(x t) + 1) / (sum x + sum t + 1), x and t [N, ...]."""

    def forward(self, input, targets):
        return autograd.seg_loss(input.reshape(input.shape[0], -1), targets, _lib.SEG_LOSS_DICE1)[3]


focal_loss = FocalLoss()
dice_loss = BinaryDiceLoss()


def calculate_seg_loss(patch_preds, mask):
    """focal(preds, mask) + dice(preds[:, 0], 1 - mask) + dice(preds[:, 1], mask) in one kernel pair (reference
    forward_utils.py:223-227); preds [B,2,S,S] probabilities, mask [B,1,S,S] or [B,S,S] of 0 / 1."""
    return autograd.seg_loss(patch_preds, mask, _lib.SEG_LOSS_ALL)[0]


def calculate_anomaly_map(patch_features: Sequence[torch.Tensor], epoch_text_feature, img_size, domain="Industrial"):
    """All tap levels in one pass: sum over levels of calculate_similarity_map(test=True)
    (what test_last.py:95-100,149 computes with 4 calls + cat + sum) -> [B,S,S]."""
    sigma, ksize = (1.0, 7) if domain == "Industrial" else (1.5, 9)
    return engine.anomaly_map(list(patch_features), epoch_text_feature, img_size, ksize, sigma)


# ------------------------------------------------------------------------------------------------
# few-shot support bank: the memory-bank score of k known-good images, added to the text-anchor map without training
SUPPORT_WEIGHT = 50.0   # derived, not tuned: the text map is 50 * (cos_1 - cos_0) + 0.5 per level (csrc/anomaly_map.hip),
#                         so one unit of cosine distance to the bank weighs as much as one unit of anchor-cosine difference


def _map_domain(domain):
    return (1.0, 7) if domain == "Industrial" else (1.5, 9)     # sigma, ksize: calculate_anomaly_map's


def build_support_bank(model, images, form=None, coreset=None, coreset_dim=128):
    """The bank of the normal images `images` ([k, 3, S, S] normalised, or a sequence of such batches): the model's unit
    seg tokens of every tap level, in image order.  form: 'fp16' / 'fp32'; None picks fp32
    for a precision="fp32" model and fp16 otherwise.  Runs under no_grad with text_embeddings=None (the IQM branch has no
    part in the bank).  coreset: None for the whole bank (an engine.SupportBank), or a ratio in (0, 1]: the greedy
    coreset of that share of the rows, selected on rows projected to coreset_dim dimensions (0: on the rows themselves)
    -- an engine.CoresetBank (engine.support_bank_coreset)."""
    if form is None:
        code = engine.dtype_code(getattr(getattr(model, "clipmodel", model), "precision", "fp32"))
        form = "fp32" if code == _lib.F32 else "fp16"
    batches = [images] if torch.is_tensor(images) else list(images)
    dev = next(model.parameters()).device
    tokens = []
    with torch.no_grad():
        for image in batches:
            if image.dtype == torch.uint8:
                raise ValueError("build_support_bank takes normalised images (engine.preprocess turns raw frames into them)")
            patch_features, _, _ = model(image.to(dev), text_embeddings=None)
            tokens.append([p.float() for p in patch_features])
    if coreset is not None:
        return engine.support_bank_coreset(tokens, form, coreset, dim=coreset_dim)
    return engine.support_bank(tokens, form)


def support_anomaly_map(patch_features: Sequence[torch.Tensor], bank, img_size, domain="Industrial", base=None,
                        weight=SUPPORT_WEIGHT, nearest=None):
    """-> [B, S, S] = base + weight * sum over levels of upsample(blur(1 - nearest cosine to the bank)), with the blur,
    align-corners upsample and level order of calculate_anomaly_map for the domain (engine.support_map).  base: the
    text-anchor map, or None for the support term alone.  nearest: a list that receives per level the int32 [B, P] index
    of the nearest bank row."""
    sigma, ksize = _map_domain(domain)
    return engine.support_map(list(patch_features), bank, img_size, ksize, sigma, base=base, weight=weight, nearest=nearest)


def _blur_upsample_host(pre, S, ksize, sigma):
    """numpy fp64: [B, g, g] -> [B, S, S], the Gaussian blur (normalised taps exp(-x^2 / 2 sigma^2), reflect border,
    rows then columns) and the bilinear align_corners=True upsample of csrc/anomaly_map.hip"""
    import numpy as np
    B, g, _ = pre.shape
    r = ksize // 2
    x = np.arange(ksize, dtype=np.float64) - r + (0.0 if ksize % 2 else 0.5)
    taps = np.exp(-(x * x) / (2.0 * sigma * sigma))
    taps /= taps.sum()
    if ksize > 1:
        at = np.arange(g)[:, None] + np.arange(ksize)[None, :] - r
        at = np.abs(at)
        at = np.where(at >= g, 2 * (g - 1) - at, at)                    # torch 'reflect'
        pre = np.einsum("byxk,k->byx", pre[:, :, at], taps)             # along x
        pre = np.einsum("bykx,k->byx", pre[:, at, :], taps)             # along y
    scale = (g - 1) / (S - 1) if S > 1 else 0.0
    s = scale * np.arange(S, dtype=np.float64)
    i0 = np.minimum(s.astype(np.int64), g - 1)
    i1 = np.minimum(i0 + 1, g - 1)
    l1 = s - i0
    l0 = 1.0 - l1
    rows = l0[None, :, None] * pre[:, i0, :] + l1[None, :, None] * pre[:, i1, :]
    return l0[None, None, :] * rows[:, :, i0] + l1[None, None, :] * rows[:, :, i1]


def support_anomaly_map_host(patch_features, bank_features, img_size, domain="Industrial", base=None,
                             weight=SUPPORT_WEIGHT, best_cos=None, nearest=None):
    """The host definition support_anomaly_map is measured against, in numpy: per level the fp64 cosines of every patch
    row ([B, P, E]) to every bank row (bank_features: per level [shots, P, E] or [N, E], fp32 rows as they are), their
    maximum per patch, d = 1 - max on the g x g grid (not clamped), then the blur, the align-corners upsample and the
    level sum in level order, and base + weight * sum; -> fp64 [B, S, S].  best_cos: per level [B * P] cosines to use
    instead of the brute force (the device's own, to check the map stage alone).  nearest: a list that receives per level
    the int64 [B, P] lowest index of the nearest bank row."""
    import numpy as np
    sigma, ksize = _map_domain(domain)
    total = None
    for l, f in enumerate(patch_features):
        f = np.asarray(f.detach().cpu() if torch.is_tensor(f) else f)
        B, P, E = f.shape
        g = int(round(P ** 0.5))
        if g * g != P:
            raise ValueError(f"{P} patches is not a square grid")
        if best_cos is not None:
            best = np.asarray(best_cos[l], np.float64).reshape(B * P)
        else:
            b = bank_features[l]
            b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, np.float64).reshape(-1, E).T
            best, idx = np.empty(B * P), np.empty(B * P, np.int64)
            q = f.reshape(B * P, E)
            for r0 in range(0, B * P, 512):
                c = q[r0:r0 + 512].astype(np.float64) @ b
                idx[r0:r0 + 512] = np.argmax(c, axis=1)
                best[r0:r0 + 512] = c.max(axis=1)
            if nearest is not None:
                nearest.append(idx.reshape(B, P))
        up = _blur_upsample_host((1.0 - best).reshape(B, g, g), img_size, ksize, sigma)
        total = up if total is None else total + up
    out = weight * total
    if base is not None:
        out = np.asarray(base.detach().cpu() if torch.is_tensor(base) else base, np.float64) + out
    return out


# ------------------------------------------------------------------------------------------------
# tiled inference: a frame of side C = S + (G - 1) * (S - O) as G x G tiles of the model's side S that overlap by O pixels
TILE_OVERLAP = 112      # derived, not tuned (no dataset was at hand): 8 grid cells of 14 px.  A tile's map is blurred over
#                         at most 9 cells -- a radius of 4 cells = 56 px, with a reflected border -- so in an overlap of
#                         112 px the half of the cross-fade where a tile's blur saw reflected cells carries less than
#                         half the weight


def tile_origins(S, G, O):
    """-> [(row, column)] of the G * G tiles' upper left corners on the canvas, tile t = i * G + j at (i * T, j * T),
    T = S - O; needs S >= 1, G >= 1 and 0 <= O <= S // 2 (then a canvas pixel lies in at most 2 tiles per axis)."""
    S, G, O = int(S), int(G), int(O)
    if S < 1 or G < 1 or not 0 <= O <= S // 2:
        raise ValueError(f"tiles: tile {S}, grid {G}, overlap {O}: tile >= 1, grid >= 1 and 0 <= overlap <= tile // 2")
    T = S - O
    return [(i * T, j * T) for i in range(G) for j in range(G)]


def tile_stitch_host(tiles, G, O):
    """The host definition engine.tile_stitch is measured against, in numpy fp64: tiles [images * G * G, ..., S, S] ->
    canvas [images, ..., C, C], C = S + (G - 1) * (S - O).  With w1(u) = min(u + 1, S - u) a tile weighs w1(y) * w1(x) at
    its (y, x); a canvas pixel under exactly one tile is that tile's value, any other is
    (sum_t w_t * v_t) / (sum_t w_t) over its covering tiles in ascending t."""
    import numpy as np
    v = np.asarray(tiles.detach().cpu() if torch.is_tensor(tiles) else tiles, np.float64)
    S = v.shape[-1]
    origins = tile_origins(S, G, O)
    if v.ndim < 3 or v.shape[-2] != S or v.shape[0] % (G * G):
        raise ValueError(f"tile_stitch_host: {v.shape} is not [images * {G * G}, ..., S, S]")
    images, lead = v.shape[0] // (G * G), v.shape[1:-2]
    C = S + (G - 1) * (S - O)
    w1 = np.minimum(np.arange(S) + 1, S - np.arange(S)).astype(np.float64)
    w = w1[:, None] * w1[None, :]
    v = v.reshape((images, G * G) + lead + (S, S))
    num, den, count = np.zeros((images,) + lead + (C, C)), np.zeros((C, C)), np.zeros((C, C), np.int64)
    single = np.zeros_like(num)
    for t, (r, c) in enumerate(origins):
        num[..., r:r + S, c:c + S] += w * v[:, t]
        den[r:r + S, c:c + S] += w
        count[r:r + S, c:c + S] += 1
        single[..., r:r + S, c:c + S] = v[:, t]
    return np.where(count == 1, single, num / den)


def image_score(det_feature: torch.Tensor, text_feature: torch.Tensor) -> torch.Tensor:
    """Per-image anomaly score (det_b . t_abnormal + 1)/2 -> [B].  Deliberate
    deviation from test_last.py:90-91, whose [B,768]@[B,768,2] broadcast yields
    [B,B,2] and then row 1; B dot products, host-side."""
    t = text_feature if text_feature.dim() == 2 else text_feature[0]
    return (det_feature @ t[:, 1].to(det_feature.device) + 1) / 2


# ------------------------------------------------------------------------------------------------
# evaluation harness counterpart (host side: numpy + sklearn, like the reference)
def _pro_curve_area(pixel_label, pixel_preds, fpr_limit, connectivity):
    """Steps 1 and 3-5 of pro_eval on scores that are normalised already: [N, H, W] arrays -> (aupro, R, N_ok, groups)"""
    import numpy as np
    from scipy import ndimage

    if connectivity not in (4, 8):
        raise ValueError(f"pro_eval: connectivity must be 4 or 8, got {connectivity}")
    if not 0.0 < float(fpr_limit) <= 1.0:
        raise ValueError(f"pro_eval: fpr_limit must lie in (0, 1], got {fpr_limit}")
    structure = np.ones((3, 3), int) if connectivity == 8 else ndimage.generate_binary_structure(2, 1)
    area = np.zeros(pixel_label.shape, np.int64)
    regions = 0
    for k in range(pixel_label.shape[0]):
        lab, count = ndimage.label(pixel_label[k] != 0, structure=structure)
        area[k] = np.bincount(lab.reshape(-1), minlength=count + 1)[lab] * (lab != 0)
        regions += count
    area = area.reshape(-1)
    n_ok = int(np.count_nonzero(area == 0))
    if regions == 0 or n_ok == 0:
        raise ValueError(f"pro_eval: {regions} regions and {n_ok} normal pixels; the PRO curve needs both")
    scores = pixel_preds.reshape(-1)
    order = np.argsort(scores, kind="stable")[::-1]
    scores, area = scores[order], area[order]
    end = np.ones(scores.size, bool)                       # last element of its tie group, walking down (-0 == +0)
    end[:-1] = scores[:-1] != scores[1:]
    weight = np.divide(1.0, area.astype(np.float64), out=np.zeros(area.size, np.float64), where=area != 0)
    fp = np.cumsum(area == 0)[end]
    x = np.concatenate([[0.0], fp.astype(np.float64) / float(n_ok)])
    y = np.concatenate([[0.0], np.minimum(1.0, np.cumsum(weight)[end] / float(regions))])
    k = int(np.count_nonzero(x <= fpr_limit))              # x ascends: the points up to the limit are a prefix
    total = float(np.sum(0.5 * (x[1:k] - x[:k - 1]) * (y[1:k] + y[:k - 1])))
    if k < x.size and x[k - 1] < fpr_limit:
        y_limit = y[k - 1] + (y[k] - y[k - 1]) * ((fpr_limit - x[k - 1]) / (x[k] - x[k - 1]))
        total += 0.5 * (fpr_limit - x[k - 1]) * (y_limit + y[k - 1])
    return float(total / fpr_limit), regions, n_ok, int(end.sum())


def _pro_shapes(pixel_label, pixel_preds):
    """maps [N, H, W] ([N, 1, H, W] and square [N, pixels] as in metrics_eval) and the labels in the same shape"""
    import numpy as np
    if pixel_preds.ndim == 4 and pixel_preds.shape[1] == 1:
        pixel_preds = pixel_preds[:, 0]
    elif pixel_preds.ndim == 2:
        side = int(pixel_preds.shape[1] ** 0.5)
        if side * side == pixel_preds.shape[1]:
            pixel_preds = pixel_preds.reshape(pixel_preds.shape[0], side, side)
    if pixel_preds.ndim != 3 or pixel_label.size != pixel_preds.size:
        raise ValueError(f"pro_eval: maps of [N, H, W] and as many labels, got {pixel_preds.shape} and {pixel_label.shape}")
    return pixel_label.reshape(pixel_preds.shape), pixel_preds


def pro_eval(pixel_label, pixel_preds, fpr_limit=0.3, connectivity=8):
    """The per-region overlap curve integrated up to the false-positive rate fpr_limit, divided by it (AUPRO), of one
    class on the host, over every distinct score -- no threshold grid.  The definition the device path is measured
    against (engine.pro_metrics):
      1. the connected components (scipy.ndimage.label; connectivity 8 = the 3x3 structure of the MVTec evaluation, or
         4) of the non-zero labels of every image on its own: R regions, area(p) = the size of p's region, N_ok normal
         pixels; R = 0 or N_ok = 0 raises ValueError
      2. the scores are min-max normalised as metrics_eval does it (in their own dtype, skipped when max == 1);
         non-finite scores and max == min raise ValueError
      3. over the groups of equal scores from the highest down: fp = normal pixels so far, S = fp64 sum of 1 / area over
         the anomalous pixels so far, the point (fp / N_ok, min(1, S / R)), with (0, 0) in front
      4. the trapezoids of the points with x <= fpr_limit, plus the one up to the linearly interpolated point at
         fpr_limit when the next point lies beyond it and the last one below it
      5. divided by fpr_limit.
    -> the unrounded AUPRO (float)."""
    return pro_eval_record(pixel_label, pixel_preds, fpr_limit, connectivity)[0]


def pro_eval_record(pixel_label, pixel_preds, fpr_limit=0.3, connectivity=8):
    """pro_eval with its integers: -> (aupro, regions, normal pixels, tie groups)"""
    import numpy as np
    pixel_preds = np.asarray(pixel_preds)
    pixel_label = np.asarray(pixel_label)
    if not np.isfinite(pixel_preds).all():
        raise ValueError("pro_eval: the scores are not all finite")
    if pixel_preds.max() == pixel_preds.min():
        raise ValueError("pro_eval: all scores are equal (max == min): the min-max normalisation divides by zero")
    if pixel_preds.max() != 1:
        pixel_preds = (pixel_preds - pixel_preds.min()) / (pixel_preds.max() - pixel_preds.min())
    pixel_label, pixel_preds = _pro_shapes(pixel_label, pixel_preds)
    return _pro_curve_area(pixel_label, pixel_preds, fpr_limit, connectivity)


def pro_eval_device(pixel_label, pixel_preds, fpr_limit=0.3, connectivity=8):
    """pro_eval on the GPU (csrc/regions.hip through engine.pro_metrics): device tensors, fp32 maps [N, H, W] (or
    [N, 1, H, W]) and labels whose non-zero entries are the anomalous pixels; the same definition and ValueErrors."""
    engine.require_gpu(pixel_preds, "pro_eval_device")
    engine.require_gpu(pixel_label, "pro_eval_device")
    pp = pixel_preds.to(torch.float32).contiguous()
    if pp.dim() == 4 and pp.shape[1] == 1:
        pp = pp[:, 0]
    if pp.dim() != 3 or pixel_label.numel() != pp.numel():
        raise ValueError(f"pro_eval_device: maps of [N, H, W] and as many labels, got {tuple(pp.shape)} and "
                         f"{tuple(pixel_label.shape)}")
    pl = pixel_label if pixel_label.dtype == torch.uint8 else (pixel_label != 0).to(torch.uint8)
    return engine.pro_metrics(pp, pl.reshape(pp.shape), fpr_limit=fpr_limit, connectivity=connectivity).aupro


def f1max_eval(labels, scores):
    """The exact F1-max of one class on the host and its operating point -- the definition the device path is measured
    against (engine.f1max_metrics).  labels 0 / non-zero and scores of one size, taken as they are (metrics_eval hands
    in the normalised ones):
      1. a stable descending argsort; a tie group ends where the next score differs (-0.0 == +0.0)
      2. after group g: tp_g = positives with a score >= the group's, m_g = all elements with one,
         F1_g = 2 tp_g / (m_g + P) with P the number of positives (= 2pr / (p + r) wherever that is defined)
      3. the maximum over the groups; a beats b iff tp_a (m_b + P) > tp_b (m_a + P) -- the groups whose fp64 F1 lies
         within 1e-9 of the fp64 maximum are compared in Python integers, so this is exact at any size -- and among groups
         of exactly equal F1 the one with the highest score wins (fewest elements flagged)
      4. threshold = that group's score, predicted = score >= threshold.
    Raises ValueError when the labels hold one class only or a score is not finite.
    -> engine.F1Max(f1, threshold, tp, fp, fn, precision, recall, groups)"""
    import numpy as np
    scores = np.asarray(scores).reshape(-1)
    positive = np.asarray(labels).reshape(-1) != 0
    if scores.size != positive.size:
        raise ValueError(f"f1max_eval: {positive.size} labels for {scores.size} scores")
    P = int(np.count_nonzero(positive))
    if P == 0 or P == positive.size:
        raise ValueError("f1max_eval: only one class present in the labels; F1 is not defined")
    if not np.isfinite(scores).all():
        raise ValueError("f1max_eval: the scores are not all finite")
    order = np.argsort(scores, kind="stable")[::-1]
    scores, positive = scores[order], positive[order]
    end = np.ones(scores.size, bool)                       # last element of its tie group, walking down
    end[:-1] = scores[:-1] != scores[1:]
    tp = np.cumsum(positive, dtype=np.int64)[end]
    m = np.flatnonzero(end).astype(np.int64) + 1
    f1 = 2.0 * tp.astype(np.float64) / (m + P).astype(np.float64)
    best = None
    for g in np.flatnonzero(f1 >= f1.max() - 1e-9):        # ascending g = descending score: the first of equals stays
        cand = (int(tp[g]), int(m[g]) + P, int(g))
        if best is None or cand[0] * best[1] > best[0] * cand[1]:
            best = cand
    g = best[2]
    threshold = scores[np.flatnonzero(end)[g]] + scores.dtype.type(0)      # -0.0 + 0.0 = +0.0, as the keys treat it
    return engine.f1max_from_counts(best[0], int(m[g]) - best[0], P, float(threshold), int(end.sum()))


def f1max_eval_device(labels, scores):
    """f1max_eval on the GPU (csrc/metrics.hip through engine.f1max_metrics): device tensors, fp32 scores taken as they
    are and labels whose non-zero entries are the positives; the same definition, ValueErrors and F1Max."""
    engine.require_gpu(scores, "f1max_eval_device")
    engine.require_gpu(labels, "f1max_eval_device")
    lab = labels if labels.dtype == torch.uint8 else (labels != 0).to(torch.uint8)
    return engine.f1max_metrics(scores.to(torch.float32).contiguous(), lab, normalise=False)[1]


PIXEL_F1_COL, IMAGE_F1_COL = "pixel F1-max", "image F1-max"
DEFECT_COLS = ["region recall", "region precision", "false regions / image"]
HostRegionTable = collections.namedtuple("HostRegionTable", "rows image_offsets record kept_mask")


def region_table_host(mask, scores, other=None, min_area=1, connectivity=8):
    """The table of the connected regions of a mask on the host -- the definition the device path is measured against
    (engine.region_table).  mask [N, H, W] (non-zero = set), scores of the same shape, taken as they are, other an
    optional second mask:
      1. scipy.ndimage.label of every image on its own (connectivity 8 = the 3x3 structure, or 4): its label numbers
         are the order of the regions' first pixels in row-major order
      2. per region: area, the bounding box of find_objects (x0 / y0 inclusive, x1 / y1 exclusive), the number of its
         pixels where other is non-zero, and over its pixels IN ROW-MAJOR ORDER peak = np.max and the position of the
         FIRST np.argmax -- the lowest flat index among equal scores; -0.0 counts as +0.0.  scipy's maximum_position
         is not used: on a constant region it returns the last pixel, not the first
      3. regions of fewer than min_area pixels get no row; the labels of the others stay what they were.
    -> HostRegionTable(rows int32 [R, 12] in engine.REGION_ROW_FIELDS' order with the fp32 bits of the peak, image_offsets
    int32 [N + 1], record (kept, regions, kept regions with overlap > 0, 0), kept_mask uint8)."""
    import numpy as np
    from scipy import ndimage

    mask, scores = np.asarray(mask), np.asarray(scores)
    if mask.ndim != 3 or scores.shape != mask.shape or (other is not None and np.asarray(other).shape != mask.shape):
        raise ValueError(f"region_table_host: a mask of [N, H, W], scores and other in its shape, got {mask.shape}")
    if connectivity not in (4, 8):
        raise ValueError(f"region_table_host: connectivity must be 4 or 8, got {connectivity}")
    if int(min_area) < 1:
        raise ValueError(f"region_table_host: min_area must be at least 1, got {min_area}")
    other = None if other is None else np.asarray(other) != 0
    structure = np.ones((3, 3), int) if connectivity == 8 else ndimage.generate_binary_structure(2, 1)
    N, H, W = mask.shape
    rows, offsets, regions, hit = [], [0], 0, 0
    kept_mask = np.zeros(mask.shape, np.uint8)
    for k in range(N):
        lab, count = ndimage.label(mask[k] != 0, structure=structure)
        regions += count
        areas = np.bincount(lab.reshape(-1), minlength=count + 1)
        for j, box in enumerate(ndimage.find_objects(lab), start=1):
            area = int(areas[j])
            if area < min_area:
                continue
            inside = lab[box] == j
            ys, xs = np.nonzero(inside)                       # row-major order
            values = scores[k][box][inside] + scores.dtype.type(0)      # -0.0 + 0.0 = +0.0
            at = int(np.argmax(values))                       # the first of equal maxima
            y0, x0 = box[0].start, box[1].start
            overlap = int(np.count_nonzero(other[k][box][inside])) if other is not None else 0
            hit += overlap > 0
            rows.append((k, j, (y0 + int(ys[0])) * W + x0 + int(xs[0]), area, x0, y0, box[1].stop, box[0].stop,
                         x0 + int(xs[at]), y0 + int(ys[at]), int(np.float32(values[at]).view(np.uint32)), overlap))
            kept_mask[k][box][inside] = 1
        offsets.append(len(rows))
    table = np.array(rows, dtype=np.int64).reshape(-1, 12).astype(np.uint32).view(np.int32)
    return HostRegionTable(table, np.array(offsets, np.int32), (len(rows), regions, hit, 0), kept_mask)


region_rows_per_image = engine.region_rows_per_image


def defects_from_record(record):
    """The three region-level columns from the six integers {predicted regions, predicted hit, gt regions, gt hit,
    images, images with a predicted region}: each ONE division of Python integers, so the host and the device path,
    which agree on the integers, agree on the bits."""
    predicted, predicted_hit, truth, truth_hit, images, _ = (int(v) for v in record)
    return {"region recall": truth_hit / truth if truth else 0.0,
            "region precision": predicted_hit / predicted if predicted else 0.0,
            "false regions / image": (predicted - predicted_hit) / images}


def _defect_shapes(masks, preds, what):
    if preds.ndim == 4 and preds.shape[1] == 1:
        preds = preds[:, 0]
    if preds.ndim != 3 or masks.size != preds.size:
        raise ValueError(f"{what}: maps of [N, H, W] and as many labels, got {preds.shape} and {masks.shape}")
    return masks.reshape(preds.shape), preds


def defects_eval(masks, preds, threshold, min_area=1):
    """The defect instances of one class at an operating point, on the host (8-connectivity): predicted = preds >=
    threshold (preds are taken as they are: metrics_eval hands in the normalised maps), its regions of at least min_area
    pixels tabulated against the ground truth `masks`, and the ground-truth regions against the KEPT predicted pixels.
    -> a dict: "region recall" = gt regions with >= 1 kept predicted pixel / gt regions, "region precision" = kept
    predicted regions with >= 1 gt pixel / kept predicted regions (0.0 without any), "false regions / image" = kept
    predicted regions without a gt pixel / images; "record" = the six integers of defects_from_record; "predicted" and
    "truth" = the per-image lists of region_rows_per_image; "kept mask" = the predicted mask without small regions."""
    import numpy as np
    masks, preds = _defect_shapes(np.asarray(masks), np.asarray(preds), "defects_eval")
    predicted = region_table_host(preds >= preds.dtype.type(threshold), preds, other=masks, min_area=min_area)
    truth = region_table_host(masks, preds, other=predicted.kept_mask)
    with_any = int(np.count_nonzero(np.diff(predicted.image_offsets)))
    record = (predicted.record[0], predicted.record[2], truth.record[0], truth.record[2], preds.shape[0], with_any)
    out = defects_from_record(record)
    out.update(record=record, predicted=region_rows_per_image(predicted.rows, predicted.image_offsets),
               truth=region_rows_per_image(truth.rows, truth.image_offsets))
    out["kept mask"] = predicted.kept_mask
    return out


def defects_eval_device(masks, preds, threshold, min_area=1, range_record=None):
    """defects_eval on the GPU (csrc/region_table.hip through engine.defects_at_threshold): fp32 device maps [N, H, W],
    labels whose non-zero entries are the anomalous pixels; threshold a number or the device record of
    engine.metrics_f1max; range_record (engine.metrics_range's) normalises raw maps on the fly.  The same dict, with
    "kept mask" a device tensor."""
    engine.require_gpu(preds, "defects_eval_device")
    engine.require_gpu(masks, "defects_eval_device")
    pp = preds.to(torch.float32).contiguous()
    if pp.dim() == 4 and pp.shape[1] == 1:
        pp = pp[:, 0]
    if pp.dim() != 3 or masks.numel() != pp.numel():
        raise ValueError(f"defects_eval_device: maps of [N, H, W] and as many labels, got {tuple(pp.shape)} and "
                         f"{tuple(masks.shape)}")
    gt = masks if masks.dtype == torch.uint8 else (masks != 0).to(torch.uint8)
    d = engine.defects_at_threshold(pp, threshold, range_record, gt_mask=gt.reshape(pp.shape), min_area=min_area)
    record = tuple(int(v) for v in d.record.cpu())
    out = defects_from_record(record)
    out.update(record=record, predicted=engine.region_table_host(d.predicted), truth=engine.region_table_host(d.truth))
    out["kept mask"] = d.mask
    return out


def _defect_columns(row, details, d, want_masks):
    for col in DEFECT_COLS:
        row[col] = d[col]
    if details is not None:
        details["defects"] = d["predicted"]
        if want_masks:
            details["kept masks"] = d["kept mask"]


# ------------------------------------------------------------------------------------------------
# bootstrap intervals of AUROC / AP over the images of one class ("Bootstrap intervals on the device")
BOOTSTRAP_COLS = ["pixel AUC", "pixel AP", "image AUC", "image AP"]
BOOTSTRAP_MAX_INVALID = 0.05    # share of a class's replicates that may lack a label before the class is refused
Bootstrap = collections.namedtuple("Bootstrap", "num P N ap valid auroc")


def bootstrap_interval_cols(cols=BOOTSTRAP_COLS):
    """the columns that metrics_eval(bootstrap=...) adds: "<column> lo", "<column> hi" for every bootstrapped column"""
    return [f"{c} {end}" for c in cols for end in ("lo", "hi")]


def bootstrap_counts(images: int, R: int, seed: int, class_index: int, image_label=None):
    """-> uint8 [R, images]: how often replicate r draws image i, `images` draws with replacement per replicate, from
    numpy's default_rng([seed, class_index]) -- the same seed, class index and image count give the same counts.
    image_label given (the stratified form): the label-0 images and the label-1 images are drawn separately, in that
    order from the one generator, each group keeping its size.  ValueError for a count above 255."""
    import numpy as np
    images, R = int(images), int(R)
    if images < 1 or R < 1:
        raise ValueError(f"bootstrap_counts: {images} images and {R} replicates; both must be at least 1")
    rng = np.random.default_rng([int(seed), int(class_index)])
    counts = np.zeros((R, images), np.int64)
    if image_label is None:
        groups = [np.arange(images)]
    else:
        lab = np.asarray(image_label).reshape(-1) != 0
        if lab.size != images:
            raise ValueError(f"bootstrap_counts: {lab.size} image labels for {images} images")
        groups = [np.nonzero(~lab)[0], np.nonzero(lab)[0]]
    rows = np.arange(R)[:, None]
    for members in groups:
        if members.size:
            draw = rng.integers(0, members.size, size=(R, members.size))
            np.add.at(counts, (rows, members[draw]), 1)
    if counts.max() > 255:
        raise ValueError(f"bootstrap_counts: an image was drawn {counts.max()} times; the counts are stored as uint8")
    return counts.astype(np.uint8)


def _bootstrap_check(valid, class_name, what):
    """logs the invalid replicates of a class and refuses it above BOOTSTRAP_MAX_INVALID"""
    import logging
    bad, R = int((~valid).sum()), int(valid.size)
    logging.getLogger(__name__).info("bootstrap %s (%s): %d of %d replicates invalid (one label only)", class_name, what,
                                     bad, R)
    if bad > BOOTSTRAP_MAX_INVALID * R:
        raise ValueError(f"bootstrap: {bad} of {R} replicates of class {class_name!r} ({what}) hold one label only, more "
                         f"than {BOOTSTRAP_MAX_INVALID:.0%}; draw the two labels separately (--bootstrap_stratified)")


def bootstrap_eval(labels, scores, image_of, counts, class_name=None, what="scores") -> Bootstrap:
    """The definition of the bootstrap records, in numpy: labels, scores and image_of (the image of every element) of
    one size, counts [R, images].  The elements are sorted ONCE by score, ascending and stable; replicate r gives element
    e the weight counts[r, image_of[e]].  With E(i) / M(i) the weighted positives / elements before sorted index i,
    P = E(n), Mtot = M(n), a tie group [i, i2) has tp = P - E(i), fp = (Mtot - M(i)) - tp, tp0 = P - E(i2),
    fp0 = (Mtot - M(i2)) - tp0 and adds (fp - fp0)(tp + tp0) to num (integers) and ((tp - tp0) / P)(tp / (tp + fp)) to ap
    (fp64), EXACTLY 0 where tp == tp0.  N = Mtot - P; P == 0 or N == 0 makes the replicate invalid: num = ap = 0.
    These are sklearn's roc_auc_score (num / (2 P N)) and average_precision_score of the literally repeated images.
    -> Bootstrap(num, P, N, ap, valid, auroc) of arrays [R]; num is int64: the weighted size of every replicate is
    checked to lie below 2^31, so num < 2^61.
    class_name: given, the invalid replicates are logged and more than 5 % of them raise ValueError."""
    import numpy as np
    labels = np.asarray(labels).reshape(-1) != 0
    scores = np.asarray(scores).reshape(-1)
    image_of = np.asarray(image_of).reshape(-1).astype(np.int64)
    counts = np.asarray(counts)
    if counts.ndim != 2 or counts.min() < 0 or counts.max() > 255:
        raise ValueError("bootstrap_eval: counts must be [R, images] in 0 .. 255")
    n, (R, images) = scores.size, counts.shape
    if labels.size != n or image_of.size != n or n < 1 or image_of.min() < 0 or image_of.max() >= images:
        raise ValueError("bootstrap_eval: labels, scores and image_of must have one size and name images of the counts")
    counts = counts.astype(np.int64)
    if int((counts * np.bincount(image_of, minlength=images)[None, :]).sum(axis=1).max()) >= 2 ** 31:
        raise ValueError("bootstrap_eval: a replicate weighs 2^31 elements or more")
    order = np.argsort(scores, kind="stable")
    s, lab, img = scores[order], labels[order].astype(np.int64), image_of[order]
    start = np.nonzero(np.concatenate([[True], s[1:] != s[:-1]]))[0]
    stop = np.concatenate([start[1:], [n]])
    num, P, N, ap = np.zeros(R, np.int64), np.zeros(R, np.int64), np.zeros(R, np.int64), np.zeros(R, np.float64)
    block = max(1, (1 << 22) // n)
    for r0 in range(0, R, block):
        w = counts[r0:r0 + block][:, img]                                        # [b, n]
        zero = np.zeros((w.shape[0], 1), np.int64)
        M = np.concatenate([zero, np.cumsum(w, axis=1)], axis=1)
        E = np.concatenate([zero, np.cumsum(w * lab[None, :], axis=1)], axis=1)
        Pb, Mt = E[:, -1:], M[:, -1:]
        tp, tp0 = Pb - E[:, start], Pb - E[:, stop]
        fp, fp0 = (Mt - M[:, start]) - tp, (Mt - M[:, stop]) - tp0
        nb = ((fp - fp0) * (tp + tp0)).sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            terms = ((tp - tp0) / Pb.astype(np.float64)) * (tp / (tp + fp).astype(np.float64))
        terms[tp == tp0] = 0.0
        ok = (Pb[:, 0] > 0) & (Mt[:, 0] - Pb[:, 0] > 0)
        P[r0:r0 + block], N[r0:r0 + block] = Pb[:, 0], Mt[:, 0] - Pb[:, 0]
        num[r0:r0 + block] = np.where(ok, nb, 0)
        ap[r0:r0 + block] = np.where(ok, terms.sum(axis=1), 0.0)
    return _bootstrap_result(num, P, N, ap, class_name, what)


def _bootstrap_result(num, P, N, ap, class_name, what) -> Bootstrap:
    import numpy as np
    valid = (P > 0) & (N > 0)
    auroc = np.where(valid, num.astype(np.float64) / np.maximum(2.0 * P * N, 1.0), 0.0)
    if class_name is not None:
        _bootstrap_check(valid, class_name, what)
    return Bootstrap(num, P, N, ap, valid, auroc)


def bootstrap_eval_device(labels, scores, per_image, counts, normalise=False, class_name=None, what="scores") -> Bootstrap:
    """bootstrap_eval on the GPU (engine.bootstrap_metrics: one sort, then csrc/bootstrap.hip) for device tensors whose
    image i owns the elements [i * per_image, (i + 1) * per_image): the same integers, ap within rounding of the order
    of its fp64 sum."""
    b = engine.bootstrap_metrics(scores, labels, per_image, counts, normalise=normalise)
    return _bootstrap_result(b.num, b.P, b.N, b.ap, class_name, what)


def bootstrap_interval(values, valid, level=0.95):
    """-> (lo, hi): numpy's default quantiles (1 - level) / 2 and (1 + level) / 2 of the valid replicates' values"""
    import numpy as np
    values, valid = np.asarray(values, np.float64), np.asarray(valid, bool)
    if not 0.0 < float(level) < 1.0:
        raise ValueError(f"bootstrap_interval: level must lie in (0, 1), got {level}")
    if not valid.any():
        raise ValueError("bootstrap_interval: no valid replicate")
    lo, hi = np.quantile(values[valid], [(1.0 - level) / 2.0, (1.0 + level) / 2.0])
    return float(lo), float(hi)


def _bootstrap_settings(bootstrap):
    known = {"R", "seed", "level", "stratified", "class_index"}
    if not isinstance(bootstrap, dict) or "R" not in bootstrap or set(bootstrap) - known:
        raise ValueError(f"bootstrap must be a dict with R and any of {sorted(known - {'R'})}")
    R, level = int(bootstrap["R"]), float(bootstrap.get("level", 0.95))
    if R < 1 or not 0.0 < level < 1.0:
        raise ValueError("bootstrap: R must be at least 1 and level must lie in (0, 1)")
    return R, int(bootstrap.get("seed", 0)), level, bool(bootstrap.get("stratified", False)), int(bootstrap.get("class_index", 0))


def _bootstrap_columns(row, details, bootstrap, class_name, image_label, replicates):
    """The interval columns of one class.  replicates(counts) -> (pixel Bootstrap, image Bootstrap or None).  A replicate
    counts where it is valid for the pixels AND for the images; the columns of a point estimate that is the fixed 0 of a
    one-label class are 0.  details (a dict or None) receives "bootstrap"."""
    import numpy as np
    R, seed, level, stratified, class_index = _bootstrap_settings(bootstrap)
    image_label = np.asarray(image_label).reshape(-1)
    counts = bootstrap_counts(image_label.size, R, seed, class_index, image_label if stratified else None)
    pixel, image = replicates(counts)
    valid = pixel.valid if image is None else pixel.valid & image.valid
    zeros = np.zeros(R, np.float64)
    arrays = {"pixel AUC": pixel.auroc, "pixel AP": pixel.ap,
              "image AUC": zeros if image is None else image.auroc, "image AP": zeros if image is None else image.ap}
    for col in BOOTSTRAP_COLS:
        fixed = image is None and col.startswith("image")
        lo, hi = (0.0, 0.0) if fixed else bootstrap_interval(arrays[col], valid, level)
        row[col + " lo"], row[col + " hi"] = round(lo, 4) * 100, round(hi, 4) * 100
    if details is not None:
        details["bootstrap"] = dict({c: np.where(valid, arrays[c], 0.0) for c in BOOTSTRAP_COLS}, valid=valid, seed=seed,
                                    R=R, level=level, stratified=stratified, class_index=class_index,
                                    images=int(image_label.size), point={c: row[c] for c in BOOTSTRAP_COLS})


def metrics_eval(pixel_label, image_label, pixel_preds, image_preds, class_names, domain, fpr_limit=None,
                 f1_max=False, details=None, defects=None, bootstrap=None):
    """Pixel / image AUROC and AP of one class, reference forward_utils.py:233-308:
    global min-max normalisation of maps and image scores (:246-253), per-image maximum of
    the normalised map (:277), Industrial score = 0.5*max_pixel + 0.5*image score, Medical =
    max_pixel (:279-282), sklearn roc_auc_score / average_precision_score (:288-296).
    `image_preds` is the per-image score vector [N] (this build computes the intended
    (det . t_abnormal + 1)/2 score; the reference's [N,2] broadcast quirk, of which it keeps
    column 0, is documented in DESIGN.md and accepted here too).
    fpr_limit: None returns the reference's dict; a number adds "pixel AUPRO", pro_eval up to that false-positive rate.
    f1_max: True adds "pixel F1-max" and "image F1-max" (f1max_eval of the normalised pixels and of the combined image
    scores; the image one is 0 where image AUC is); details: a dict that then receives "pixel threshold" and "image
    threshold" (None where the column is 0), in normalised units, and -- when it holds a true "masks" on entry -- the
    uint8 predicted masks `normalised map >= pixel threshold` under "masks".
    defects: None, or a min_area >= 1 (needs f1_max=True): adds DEFECT_COLS -- "region recall", "region precision", "false
    regions / image" of defects_eval at the pixel threshold -- and puts the per-image lists of the kept predicted regions
    under details["defects"] and, where "masks" was asked for, the filtered masks under details["kept masks"].
    bootstrap: None, or dict(R=, seed=0, level=0.95, stratified=False, class_index=0): R replicates of the class's images
    (bootstrap_counts) through bootstrap_eval -- slow on the host, meant for small classes -- add "<column> lo" and
    "<column> hi" for the four columns above (bootstrap_interval_cols), in percent with the table's rounding, 0 where
    the point estimate is the fixed 0; the scores are the normalised pixels and the combined image scores of the WHOLE
    class, not re-normalised per replicate.  details["bootstrap"] receives the replicate arrays and the valid mask."""
    import numpy as np
    from sklearn.metrics import average_precision_score, roc_auc_score

    if defects is not None and not f1_max:
        raise ValueError("metrics_eval: defects needs f1_max=True (the regions are those at its pixel threshold)")

    # arithmetic stays in the callers' dtype (float32 arrays in test_last.py), as in the reference: the min-max
    # normalisation decides which pixels tie, and ties decide AUROC / AP digits
    pixel_preds = np.asarray(pixel_preds)
    image_preds = np.asarray(image_preds)
    pixel_label = np.asarray(pixel_label)
    image_label = np.asarray(image_label)
    if pixel_preds.max() != 1:
        pixel_preds = (pixel_preds - pixel_preds.min()) / (pixel_preds.max() - pixel_preds.min())
    if image_preds.max() != 1:
        image_preds = (image_preds - image_preds.min()) / (image_preds.max() - image_preds.min())
    if pixel_preds.ndim == 4 and pixel_preds.shape[1] == 1:
        pixel_preds = pixel_preds[:, 0]
    elif pixel_preds.ndim == 2:                      # [N, pixels] -> [N, side, side] (:261-267)
        side = int(pixel_preds.shape[1] ** 0.5)
        if side * side == pixel_preds.shape[1]:
            pixel_preds = pixel_preds.reshape(pixel_preds.shape[0], side, side)
    if image_preds.ndim == 2 and image_preds.shape[1] == 2:
        image_preds = image_preds[:, 0]
    elif image_preds.ndim > 1:
        image_preds = image_preds.reshape(-1)
    pmax = pixel_preds.max(axis=(1, 2))
    image_preds = pmax * 0.5 + image_preds * 0.5 if domain != "Medical" else pmax
    pl, pp = pixel_label.reshape(-1), pixel_preds.reshape(-1)
    pixel_auc = roc_auc_score(pl, pp)
    pixel_ap = average_precision_score(pl, pp)
    if image_label.max() != image_label.min():
        il = image_label.reshape(-1)
        image_auc = roc_auc_score(il, image_preds.reshape(-1))
        image_ap = average_precision_score(il, image_preds.reshape(-1))
    else:
        image_auc = image_ap = 0
    row = {"class name": class_names, "pixel AUC": round(pixel_auc, 4) * 100, "pixel AP": round(pixel_ap, 4) * 100,
           "image AUC": round(image_auc, 4) * 100, "image AP": round(image_ap, 4) * 100}
    if fpr_limit is not None:      # the maps are normalised above: max == 1 now, or they were taken as they are
        row["pixel AUPRO"] = round(_pro_curve_area(*_pro_shapes(pixel_label, pixel_preds), fpr_limit, 8)[0], 4) * 100
    if f1_max:
        pixel_f1 = f1max_eval(pl, pp)
        image_f1 = f1max_eval(image_label.reshape(-1), image_preds.reshape(-1)) if image_label.max() != image_label.min() else None
        _f1_columns(row, details, pixel_f1, image_f1)
        want_masks = details is not None and details.get("masks") is True
        if want_masks:
            details["masks"] = (pixel_preds >= pixel_preds.dtype.type(pixel_f1.threshold)).astype(np.uint8)
        if defects is not None:
            _defect_columns(row, details, defects_eval(pixel_label, pixel_preds, pixel_f1.threshold, defects), want_masks)
    if bootstrap is not None:
        def replicates(counts):
            image_of = np.repeat(np.arange(pixel_preds.shape[0]), pp.size // pixel_preds.shape[0])
            pixel = bootstrap_eval(pl, pp, image_of, counts, class_names, "pixels")
            if image_label.max() == image_label.min():
                return pixel, None
            return pixel, bootstrap_eval(image_label.reshape(-1), image_preds.reshape(-1), np.arange(image_label.size),
                                         counts, class_names, "images")
        _bootstrap_columns(row, details, bootstrap, class_names, image_label, replicates)
    return row


def _f1_columns(row, details, pixel_f1, image_f1):
    row[PIXEL_F1_COL] = round(pixel_f1.f1, 4) * 100
    row[IMAGE_F1_COL] = round(image_f1.f1 if image_f1 is not None else 0, 4) * 100
    if details is not None:
        details["pixel threshold"] = pixel_f1.threshold
        details["image threshold"] = None if image_f1 is None else image_f1.threshold


def metrics_eval_device(pixel_label, image_label, pixel_preds, image_preds, class_names, domain, fpr_limit=None,
                        f1_max=False, details=None, defects=None, bootstrap=None):
    """metrics_eval with the sort and the curve sums on the GPU (csrc/metrics.hip through engine.curve_metrics): the same
    arguments, shape handling, domain rule, `image_label.max() != image_label.min()` rule, result dict and rounding, and
    the same numbers -- sklearn's tie groups and definitions, an integer AUROC numerator, an fp64 AP sum.
    pixel_preds (fp32) and pixel_label (uint8 0 / 1, or anything whose non-zero entries are the positives) are device
    tensors; the per-image arrays may live anywhere.  Raises ValueError where metrics_eval does (one pixel class only,
    non-finite scores) and where the reference's normalisation divides by zero (all scores equal).
    fpr_limit: as in metrics_eval, with "pixel AUPRO" from engine.pro_metrics (a labelling, a second sort, the PRO curve).
    f1_max, details: as in metrics_eval; the columns come from engine.f1max_metrics, that is from the ONE sort that
    serves AUROC / AP already, and details["masks"] is a device tensor from engine.metrics_threshold, which normalises
    the raw maps on the fly and reads the threshold from the device record.
    defects: as in metrics_eval, through engine.defects_at_threshold: the threshold and the range stay on the device, the
    lists come from the region tables and details["kept masks"] is a device tensor.
    bootstrap: as in metrics_eval, through engine.bootstrap_metrics: one more sort per level (pixels, images) with the
    image index as payload, then the weighted curve pass of csrc/bootstrap.hip over all R replicates."""
    import numpy as np

    if defects is not None and not f1_max:
        raise ValueError("metrics_eval_device: defects needs f1_max=True (the regions are those at its pixel threshold)")
    engine.require_gpu(pixel_preds, "metrics_eval_device")
    engine.require_gpu(pixel_label, "metrics_eval_device")
    dev = pixel_preds.device
    n_img = pixel_preds.shape[0]
    pp = pixel_preds.to(torch.float32).contiguous()
    pl = pixel_label if pixel_label.dtype == torch.uint8 else (pixel_label != 0).to(torch.uint8)
    records, pixel_f1, image_f1 = {}, None, None
    if f1_max:
        pixel, pixel_f1 = engine.f1max_metrics(pp, pl, per_image=pp.numel() // n_img, records=records)
    else:
        pixel = engine.curve_metrics(pp, pl, per_image=pp.numel() // n_img)
    image_label = np.asarray(image_label.cpu() if torch.is_tensor(image_label) else image_label)
    if image_label.max() != image_label.min():
        ip = torch.as_tensor(image_preds).to(device=dev, dtype=torch.float32).contiguous()
        rng, _ = engine.metrics_range(ip)
        r = engine.metrics_range_host(rng)
        if r["nonfinite"] or r["max"] == r["min"]:
            raise ValueError("metrics_eval_device: image scores are not finite or all equal")
        ip = engine.metrics_normalise(ip, rng)
        if ip.dim() == 2 and ip.shape[1] == 2:
            ip = ip[:, 0]
        ip = ip.reshape(-1)
        score = pixel.image_max * 0.5 + ip * 0.5 if domain != "Medical" else pixel.image_max
        il = torch.as_tensor(image_label.reshape(-1) != 0).to(device=dev, dtype=torch.uint8)
        if f1_max:
            image, image_f1 = engine.f1max_metrics(score, il, normalise=False)
        else:
            image = engine.curve_metrics(score, il, normalise=False)
        image_auc, image_ap = image.auroc, image.ap
    else:
        image_auc = image_ap = 0
    row = {"class name": class_names, "pixel AUC": round(pixel.auroc, 4) * 100, "pixel AP": round(pixel.ap, 4) * 100,
           "image AUC": round(image_auc, 4) * 100, "image AP": round(image_ap, 4) * 100}
    if fpr_limit is not None:
        row["pixel AUPRO"] = round(pro_eval_device(pl, pp, fpr_limit=fpr_limit), 4) * 100
    if f1_max:
        _f1_columns(row, details, pixel_f1, image_f1)
        want_masks = details is not None and details.get("masks") is True
        shaped = pp[:, 0] if pp.dim() == 4 and pp.shape[1] == 1 else pp
        if want_masks:
            details["masks"] = engine.metrics_threshold(shaped, records["f1max"], range_record=records["range"],
                                                        totals=False)[0]
        if defects is not None:
            if shaped.dim() == 2:                       # [N, pixels] -> [N, side, side], as metrics_eval reshapes it
                side = int(shaped.shape[1] ** 0.5)
                if side * side == shaped.shape[1]:
                    shaped = shaped.reshape(shaped.shape[0], side, side)
            _defect_columns(row, details, defects_eval_device(pl, shaped, records["f1max"], defects,
                                                              range_record=records["range"]), want_masks)
    if bootstrap is not None:
        def replicates(counts):
            pixel = bootstrap_eval_device(pl, pp, pp.numel() // n_img, counts, True, class_names, "pixels")
            if image_label.max() == image_label.min():
                return pixel, None
            return pixel, bootstrap_eval_device(il, score, 1, counts, False, class_names, "images")
        _bootstrap_columns(row, details, bootstrap, class_names, image_label, replicates)
    return row


def visualize(*args, **kwargs):
    """The reference's heat-map writer (forward_utils.py:316-360: cv2 colour maps + file output) is outside this
    build (OUT OF SCOPE).  The name exists so that `from forward_utils import visualize`
    (reference test_last.py:17-22) resolves; calling it -- `--visualize` -- says so instead of failing on cv2."""
    raise NotImplementedError("forward_utils.visualize: visualisation is outside the MI355X hot-path build; take the "
                              "[N, S, S] maps test_last.get_predictions returns and plot them with your own tooling")


# ------------------------------------------------------------------------------------------------
# heat-map overlays: the definition in numpy (engine.overlay_render / csrc/overlay.hip give the same bytes)
def _overlay_range(range_record):
    """None, the record of engine.metrics_range (int64 [3], any device, or its numpy copy) or the dict of
    engine.metrics_range_host -> None or (min, max) as np.float32"""
    import numpy as np
    if range_record is None:
        return None
    if isinstance(range_record, dict):
        return np.float32(range_record["min"]), np.float32(range_record["max"])
    r = np.ascontiguousarray(range_record.detach().cpu().numpy() if torch.is_tensor(range_record) else range_record)
    if r.dtype != np.int64 or r.size != 3:
        raise ValueError("overlays: range_record must be the int64 [3] record of engine.metrics_range")
    mn, mx = r.reshape(-1)[:1].view(np.float32)
    return mn, mx


def overlay_contour_host(mask, thickness: int):
    """bool [..., H, W]: mask != 0 where some pixel inside the image with |dy| <= T and |dx| <= T has mask == 0"""
    import numpy as np
    m = np.asarray(mask) != 0
    T = int(thickness)
    H, W = m.shape[-2:]
    near_zero = np.zeros_like(m)
    for dy in range(-T, T + 1):
        for dx in range(-T, T + 1):
            if abs(dy) >= H or abs(dx) >= W:          # the whole shifted copy lies outside the image
                continue
            ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
            xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
            near_zero[..., yd, xd] |= ~m[..., ys, xs]
    return m & near_zero if T > 0 else np.zeros_like(m)


def render_overlays_host(frames, maps, range_record=None, pred=None, truth=None, lut="jet", alpha256: int = 128,
                         thickness: int = 1, pred_colour=(255, 255, 255), truth_colour=(0, 255, 0),
                         mean=engine.CLIP_MEAN, std=engine.CLIP_STD, panels=None):
    """The definition of the overlay panels, in numpy: -> uint8 [B, n * H, W, 3], the n panels of `panels` (a non-empty
    subset of ("frame", "heat", "truth"), always in that order; None: all, without "truth" when truth is None) stacked
    vertically.  frames fp32 [B, 3, H, W], the normalised model input; maps fp32 [B, H, W]; range_record what
    engine.metrics_range gives, or None; pred / truth [B, H, W], non-zero = set, or None; lut a name of
    engine.overlay_lut or uint8 [256, 3].  Per pixel
      F[c]  = clamp(rint(((x[c] * std[c]) + mean[c]) * 255), 0, 255), every operation rounded to fp32, NaN -> 0;
      q     = trunc(min(max(n, 0), 1) * 255), the product rounded toward zero, NaN -> 0, n = engine.metrics_normalise's
              value with the record (x itself without one) -- every map is quantised, a class maximum of 1 included;
      blend(u, v) = (alpha256 * u + (256 - alpha256) * v + 128) >> 8;
      frame = F; heat = blend(F, lut[q]) with pred_colour on contour(pred); truth = blend(F, truth_colour) where
      truth != 0, else F, then truth_colour on contour(truth), then pred_colour on contour(pred)
    with contour = overlay_contour_host(mask, thickness).  Arguments may be tensors (of any device) or arrays."""
    import numpy as np
    host = lambda t: None if t is None else np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t)
    x, m, pred, truth = host(frames), host(maps), host(pred), host(truth)
    if x.dtype != np.float32 or x.ndim != 4 or x.shape[1] != 3 or m.dtype != np.float32 or m.shape != x.shape[:1] + x.shape[2:]:
        raise ValueError(f"overlays: fp32 frames [B, 3, H, W] and fp32 maps [B, H, W], got {x.shape} and {m.shape}")
    for mask in (pred, truth):
        if mask is not None and mask.shape != m.shape:
            raise ValueError(f"overlays: a mask of {mask.shape} for maps of {m.shape}")
    panels = engine.overlay_panels(panels, truth is not None)
    a, T = int(alpha256), int(thickness)
    if not 0 <= a <= 256 or not 0 <= T <= engine.OVERLAY_MAX_THICKNESS:
        raise ValueError(f"overlays: alpha256 in 0 .. 256 and thickness in 0 .. 8, got {alpha256} and {thickness}")
    table = host(engine.overlay_lut(lut) if isinstance(lut, str) else lut)
    if table.dtype != np.uint8 or table.shape != (256, 3):
        raise ValueError("overlays: lut must be uint8 [256, 3]")
    blend = lambda u, v: (a * u.astype(np.int64) + (256 - a) * np.asarray(v, np.int64) + 128) >> 8
    with np.errstate(all="ignore"):
        sd, mu = np.asarray(std, np.float32).reshape(1, 3, 1, 1), np.asarray(mean, np.float32).reshape(1, 3, 1, 1)
        v = np.rint(((x * sd) + mu) * np.float32(255))
        F = np.where(np.isnan(v), np.float32(0), np.clip(v, 0, 255)).astype(np.int64).transpose(0, 2, 3, 1)     # [B, H, W, 3]
        rng = _overlay_range(range_record)
        n = m if rng is None or rng[1] == np.float32(1) else (m - rng[0]) / (rng[1] - rng[0])
        q = np.where(np.isnan(n), 0.0, np.floor(np.clip(n, 0, 1).astype(np.float64) * 255.0)).astype(np.int64)
    pc, tc = np.asarray(pred_colour, np.int64), np.asarray(truth_colour, np.int64)
    out = []
    for name in panels:
        if name == "frame":
            img = F.copy()
        elif name == "heat":
            img = blend(F, table[q])
        else:
            img = np.where((truth != 0)[..., None], blend(F, tc), F)
            img[overlay_contour_host(truth, T)] = tc
        if name != "frame" and pred is not None:
            img[overlay_contour_host(pred, T)] = pc
        out.append(img.astype(np.uint8))
    return np.concatenate(out, axis=1)


def render_overlays(frames, maps, range_record=None, pred=None, truth=None, lut="jet", alpha256: int = 128,
                    thickness: int = 1, pred_colour=(255, 255, 255), truth_colour=(0, 255, 0), mean=engine.CLIP_MEAN,
                    std=engine.CLIP_STD, panels=None):
    """render_overlays_host's call on the GPU: device tensors in, a uint8 device tensor [B, n * H, W, 3] out, the same
    bytes (engine.overlay_render, one launch on the current stream)."""
    return engine.overlay_render(frames, maps, range_record=range_record, pred=pred, truth=truth, alpha=int(alpha256) / 256,
                                 lut=lut, thickness=thickness, panels=panels, pred_colour=pred_colour,
                                 truth_colour=truth_colour, mean=mean, std=std)


# ------------------------------------------------------------------------------------------------ PNG encoding
# The definition of engine.png_encode's bytes (csrc/png.hip, csrc/png_plan.h), in numpy and plain Python, with no zlib in
# the encoding itself.  pixels uint8 [images, H, W, C], C in {1, 3}, R = W * C:
#   filters   the filtered stream of an image is H rows of 1 + R bytes: the filter type, then the row under it; PNG's five
#             types with bpp = C, the row above row 0 all zeros.  A row takes the type with the smallest sum of
#             min(b, 256 - b) over its R filtered bytes, ties to the lowest type.
#   segments  rows_per_segment = max(1, 32768 // (1 + R)) whole rows (the last segment may be shorter), each compressed on
#             its own into one deflate block that ends on a byte; 1 + R > 32768 is refused.
#   tokens    distance-1 matches only.  A maximal run of n equal bytes inside a segment is a literal; the other n - 1
#             bytes follow in pieces of 258, and a last piece of 3 or more is a match, one of 1 or 2 is literals.
#   code      png_code_lengths_host.  The leaves are the symbols with a count, in (count, symbol) order; the two smallest
#             nodes are merged, taken from the queue of leaves and the queue of merged nodes (in the order they were made),
#             a leaf before a merged node of the same weight.  The tree gives the NUMBER of codes of every length, a leaf
#             deeper than the limit counted at the limit; while their Kraft sum exceeds 1, one code of the limit's length
#             goes and the longest shorter code becomes two codes one bit longer.  The lengths are handed out in leaf
#             order, the longest to the rarest.  Limit 15 for literals / lengths, 7 for the code-length alphabet; an
#             alphabet with fewer than two leaves is filled up with its lowest other symbols at count 0.  The distance
#             alphabet is one code (HDIST = 0): length 1 if the segment has a match, else 0.
#   lengths   the HLIT literal / length lengths and the distance length, as one sequence: a non-zero length is sent as
#             itself (symbol 16 is never used); of a zero run of z, while z >= 11 one symbol 18 takes min(z, 138), then one
#             symbol 17 takes what is left if that is 3 or more, else it is sent as symbols 0.
#   block     BFINAL = 0, BTYPE = 2, the header, the tokens, end-of-block, three zero bits (an empty stored block),
#             padding to the byte, 00 00 FF FF.  Where that is not shorter than the stored block (00, LEN, NLEN, the bytes)
#             the stored block is taken, so a segment never takes more than its length + 5 bytes.
#   stream    78 01, the segments, 03 00 (an empty final fixed block), the Adler-32 of the filtered stream, big-endian,
#             combined from the segments' sums s1 = sum b[i], s2 = sum (n - i) b[i] in segment order.
PNG_SEGMENT_BYTES = engine.PNG_SEGMENT_BYTES
_PNG_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
_PNG_LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
                    227, 258)
_PNG_LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)


def png_filter_host(image):
    """image uint8 [H, W, C] (numpy) -> the filtered stream uint8 [H, 1 + W * C]: the chosen type and the filtered bytes
    of every row."""
    import numpy as np
    image = np.asarray(image)
    H, W, C = image.shape
    R = W * C
    x = image.reshape(H, R).astype(np.int32)
    a = np.zeros_like(x)
    a[:, C:] = x[:, :-C] if R > C else 0
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, C:] = x[:-1, :-C] if R > C else 0
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    forms = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255          # [5, H, R]
    cost = np.minimum(forms, 256 - forms).sum(axis=2)                                   # [5, H]
    choice = np.argmin(cost, axis=0)                                                    # the first of equal minima
    out = np.empty((H, 1 + R), dtype=np.uint8)
    out[:, 0] = choice
    out[:, 1:] = forms[choice, np.arange(H)]
    return out


def png_code_lengths_host(counts, limit):
    """counts -> (the code length of every symbol, the number of leaves that lay deeper than the limit); see `code`"""
    keys = {s: int(c) for s, c in enumerate(counts) if c}
    for s in range(len(counts)):
        if len(keys) >= 2:
            break
        keys.setdefault(s, 0)
    order = sorted(keys, key=lambda s: (keys[s], s))
    m = len(order)
    weight = [keys[s] for s in order] + [0] * (m - 1)
    parent = [0] * (2 * m - 1)
    leaf, node = 0, m
    for nxt in range(m, 2 * m - 1):
        total = 0
        for _ in range(2):
            if leaf < m and (node >= nxt or weight[leaf] <= weight[node]):
                k, leaf = leaf, leaf + 1
            else:
                k, node = node, node + 1
            total += weight[k]
            parent[k] = nxt
        weight[nxt] = total
    depth = [0] * (2 * m - 1)
    for k in range(2 * m - 3, -1, -1):
        depth[k] = depth[parent[k]] + 1
    num = [0] * (limit + 1)
    for d in depth[:m]:
        num[min(d, limit)] += 1
    total = sum(num[n] << (limit - n) for n in range(1, limit + 1))
    while total > 1 << limit:
        num[limit] -= 1
        for n in range(limit - 1, 0, -1):
            if num[n]:
                num[n] -= 1
                num[n + 1] += 2
                break
        total -= 1
    lengths, k = [0] * len(counts), 0
    for n in range(limit, 0, -1):
        for _ in range(num[n]):
            lengths[order[k]] = n
            k += 1
    return lengths, sum(d > limit for d in depth[:m])


def _png_canonical(lengths):
    """the canonical code of every symbol, bit-reversed: deflate sends a Huffman code from its most significant bit"""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = []
    for n in lengths:
        if n == 0:
            out.append(0)
            continue
        out.append(int(format(nxt[n], f"0{n}b")[::-1], 2))
        nxt[n] += 1
    return out


def _png_length_tokens(seq):
    """how a sequence of code lengths is sent: (symbol, extra bits, extra value) per code-length token"""
    out, i, n = [], 0, len(seq)
    while i < n:
        if seq[i]:
            out.append((seq[i], 0, 0))
            i += 1
            continue
        z = 1
        while i + z < n and seq[i + z] == 0:
            z += 1
        i += z
        while z >= 11:
            take = min(z, 138)
            out.append((18, 7, take - 11))
            z -= take
        if z >= 3:
            out.append((17, 3, z - 3))
        else:
            out.extend([(0, 0, 0)] * z)
    return out


def png_tokens_host(segment):
    """segment uint8 [n] (numpy) -> (position, kind, length) arrays of its tokens in order: kind 1 a literal of the byte
    at `position`, kind 2 a distance-1 match of `length` that starts there"""
    import numpy as np
    n = segment.size
    starts = np.flatnonzero(np.concatenate(([True], segment[1:] != segment[:-1])))
    runs = np.diff(np.concatenate((starts, [n])))
    p = np.arange(n) - np.repeat(starts, runs)                     # the position in the run
    m, q = np.repeat(runs, runs) - 1, p - 1
    piece = np.where(q // 258 < m // 258, 258, m % 258)
    literal = (p == 0) | (piece < 3)
    match = ~literal & (q % 258 == 0)
    where = np.flatnonzero(literal | match)
    return where, np.where(literal[where], 1, 2), np.where(literal[where], 0, piece[where])


def _png_pack(values, widths):
    """bits, least significant first: value i takes widths[i] <= 32 bits -> (uint8 bytes, zero-padded; the bit count)"""
    import numpy as np
    values, widths = np.asarray(values, dtype=np.uint64), np.asarray(widths, dtype=np.int64)
    top = int(widths.max()) if widths.size else 0
    lanes = np.arange(top, dtype=np.uint64)
    bits = ((values[:, None] >> lanes[None, :]) & np.uint64(1)).astype(np.uint8)
    keep = np.arange(top)[None, :] < widths[:, None]
    return np.packbits(bits[keep], bitorder="little"), int(widths.sum())


def png_segment_host(segment, info=None):
    """One segment of a filtered stream (uint8 [n], numpy) -> its deflate block as uint8 bytes.  info, a dict, collects
    "stored", "huffman" (segment counts), "limited" and "cl_limited" (leaves that the limit moved up)."""
    import numpy as np
    n = segment.size
    where, kind, length = png_tokens_host(segment)
    base, extra = np.asarray(_PNG_LENGTH_BASE), np.asarray(_PNG_LENGTH_EXTRA)
    slot = np.searchsorted(base, np.where(kind == 2, length, 3), side="right") - 1
    symbol = np.where(kind == 1, segment[where].astype(np.int64), 257 + slot)
    counts = np.bincount(symbol, minlength=286)
    counts[256] += 1
    has_match = int((kind == 2).any())
    lengths, limited = png_code_lengths_host(counts, 15)
    codes = _png_canonical(lengths)
    hlit = 286
    while hlit > 257 and lengths[hlit - 1] == 0:
        hlit -= 1
    cl_tokens = _png_length_tokens(lengths[:hlit] + [has_match])
    cl_counts = [0] * 19
    for s, _, _ in cl_tokens:
        cl_counts[s] += 1
    cl_lengths, cl_limited = png_code_lengths_host(cl_counts, 7)
    cl_codes = _png_canonical(cl_lengths)
    hclen = 19
    while hclen > 4 and cl_lengths[_PNG_CL_ORDER[hclen - 1]] == 0:
        hclen -= 1
    head = [(0, 1), (2, 2), (hlit - 257, 5), (0, 5), (hclen - 4, 4)] + [(cl_lengths[s], 3) for s in _PNG_CL_ORDER[:hclen]]
    for s, eb, e in cl_tokens:
        head += [(cl_codes[s], cl_lengths[s]), (e, eb)]
    lengths_a, codes_a = np.asarray(lengths, dtype=np.int64), np.asarray(codes, dtype=np.int64)
    eb = np.where(kind == 2, extra[slot], 0)
    ev = np.where(kind == 2, length - base[slot], 0)
    value = codes_a[symbol] | (ev << lengths_a[symbol])             # a match ends in its distance code, one zero bit
    width = lengths_a[symbol] + eb + (kind == 2)
    values = np.concatenate(([v for v, _ in head], value, [codes[256], 0]))
    widths = np.concatenate(([w for _, w in head], width, [lengths[256], 3]))
    body, _ = _png_pack(values, widths)
    block = np.concatenate((body, np.array([0, 0, 255, 255], dtype=np.uint8)))
    stored = block.size >= n + 5
    if stored:
        block = np.concatenate((np.array([0, n & 255, n >> 8, ~n & 255, (~n >> 8) & 255], dtype=np.uint8), segment))
    if info is not None:
        info["stored" if stored else "huffman"] = info.get("stored" if stored else "huffman", 0) + 1
        info["limited"] = info.get("limited", 0) + limited
        info["cl_limited"] = info.get("cl_limited", 0) + cl_limited
    return block


def png_encode_host(pixels, info=None):
    """pixels uint8 [images, H, W, C] or [images, H, W] (numpy or a host tensor) -> (payload uint8 numpy, offsets: a list
    of images + 1 ints): image i's zlib stream is payload[offsets[i]:offsets[i + 1]].  The definition of
    engine.png_encode's bytes; ValueError for C outside {1, 3} and a filtered row of more than 32768 bytes."""
    import numpy as np
    pixels = pixels.numpy() if torch.is_tensor(pixels) else np.asarray(pixels)
    if pixels.ndim == 3:
        pixels = pixels[..., None]
    if pixels.dtype != np.uint8 or pixels.ndim != 4:
        raise ValueError(f"png_encode_host: pixels must be uint8 [images, H, W, C], got {pixels.dtype} {pixels.shape}")
    images, H, W, C = pixels.shape
    geom = engine.png_segments(H, W, C)
    step = geom["rows_per_segment"]
    parts, offsets = [], [0]
    for i in range(images):
        rows = png_filter_host(pixels[i])
        stream = [np.array([0x78, 0x01], dtype=np.uint8)]
        a, b = 1, 0
        for y in range(0, H, step):
            segment = rows[y:y + step].reshape(-1)
            stream.append(png_segment_host(segment, info))
            n = segment.size
            s1 = int(segment.sum(dtype=np.int64))
            s2 = int((segment.astype(np.int64) * np.arange(n, 0, -1)).sum())
            b = (b + n * a + s2) % 65521
            a = (a + s1) % 65521
        stream.append(np.array([0x03, 0x00, b >> 8, b & 255, a >> 8, a & 255], dtype=np.uint8))
        data = np.concatenate(stream)
        parts.append(data)
        offsets.append(offsets[-1] + data.size)
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)), offsets


def png_file(stream, H, W, C) -> bytes:
    """One image's zlib stream (bytes or a uint8 numpy array) -> its PNG file: the signature, IHDR (8 bit, colour type 2
    for C = 3 and 0 for C = 1, no interlace), one IDAT and IEND, each chunk with its CRC-32 (zlib.crc32 on the host: the
    compressed bytes pass through it on their way to disk anyway)."""
    import struct
    import zlib
    if C not in (1, 3):
        raise ValueError(f"png_file: C must be 1 or 3, got {C}")

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(data, zlib.crc32(tag)))

    ihdr = struct.pack(">IIBBBBB", W, H, 8, 2 if C == 3 else 0, 0, 0, 0)
    stream = stream if isinstance(stream, bytes) else bytes(memoryview(stream))
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + chunk(b"IDAT", stream) + chunk(b"IEND", b"")


def png_files(payload, offsets, H, W, C):
    """The zlib streams of engine.png_encode / png_encode_host -> one PNG file (bytes) per image (png_file).  payload:
    bytes, a numpy array or a host tensor; offsets: images + 1 integers (a list, an array or a host tensor)."""
    if torch.is_tensor(payload):
        payload = payload.numpy()
    view = memoryview(payload).cast("B") if not isinstance(payload, (bytes, bytearray)) else memoryview(payload)
    offsets = [int(o) for o in (offsets.tolist() if hasattr(offsets, "tolist") else offsets)]
    return [png_file(bytes(view[lo:hi]), H, W, C) for lo, hi in zip(offsets[:-1], offsets[1:])]
